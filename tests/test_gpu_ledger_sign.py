"""Ledger.messages and Ledger.sign (cstark_ledger_messages, cstark_ledger_sign) on batches whose nonces and balances move inside the
batch -- a sender who sends twice, a receiver who later sends, a pair in both directions -- at depth 3 and 15 with 16 transfers: the
messages are those of the witness the batch leaves; the signed batch passes the checked apply, gives the unchecked apply's witness and
proves; a flipped bit is refused at its transfer; sign refuses where apply refuses, and with KEY at the first wrong secret; the call is
read-only; a partial ledger signs the same."""
import functools

import numpy as np
import pytest

import sig_cases as SC
import sign_cases as SG

pytestmark = pytest.mark.gpu

FIELDS = ("initial_roots", "final_root", "s_old_values", "r_old_values", "s_indices", "r_indices", "s_paths", "r_paths", "deltas", "sig_rx", "sig_s")
SEED = 0x1ED6E5
# account k of a case: secret key k + 1, balance 1000, nonce k.  Transfers name accounts by k: (sender, receiver, delta)
TRANSFERS = [(0, 1, 10), (0, 2, 20),                 # a sender who sends twice (its second message carries the moved nonce)
             (1, 3, 5), (3, 1, 7),                   # a pair in both directions; 1 and 3 are receivers who later send
             (2, 0, 1020), (4, 5, 1000), (5, 4, 2000), (0, 4, 1), (4, 0, 1), (1, 2, 1012), (2, 1, 0), (3, 5, 998), (5, 3, 998), (0, 1, 1000),
             (1, 0, 1000), (2, 3, 12)]              # deltas that only the balances moved inside the batch cover
INDICES = {3: [0, 1, 6, 7, 3, 4], 15: [0, 12345, 2**15 - 1, 12344, 777, 31000]}


class Case:
    def __init__(self, depth):
        O = SC._oracle()
        self.depth = depth
        self.indices = np.array(INDICES[depth], np.uint64)
        self.account_secrets = np.arange(1, 7, dtype=np.uint64)
        self.values = np.zeros((6, 14), np.uint64)
        self.values[:, :12] = SG.public_keys(self.account_secrets)
        self.values[:, 12] = O.to_mont(np.full(6, 1000, np.uint64))
        self.values[:, 13] = O.to_mont(np.arange(6, dtype=np.uint64))
        self.s = np.array([self.indices[a] for a, _, _ in TRANSFERS], np.uint64)
        self.r = np.array([self.indices[b] for _, b, _ in TRANSFERS], np.uint64)
        self.deltas = O.to_mont(np.array([d for _, _, d in TRANSFERS], np.uint64))
        self.secrets = np.array([self.account_secrets[a] for a, _, _ in TRANSFERS], np.uint64)
        for a in (self.indices, self.account_secrets, self.values, self.s, self.r, self.deltas, self.secrets):
            a.flags.writeable = False

    @property
    def batch(self):
        return self.s, self.r, self.deltas

    def ledger(self, backend):
        from certificate_stark_amd.prover import Ledger
        led = Ledger(self.depth, backend)
        led.set_accounts(self.indices, self.values)
        return led


@functools.lru_cache(maxsize=None)
def case(depth):
    return Case(depth)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


_WITNESSES = {}


def _unsigned_witness(backend, depth):
    """the witness the batch leaves when applied with all-zero signatures (the unchecked apply copies them through); computed once per
    depth and shared, read-only"""
    if depth not in _WITNESSES:
        c = case(depth)
        led = c.ledger(backend)
        m = led.apply(c.batch + (np.zeros((16, 6), np.uint64), np.zeros((16, 32), np.uint8)))
        led.close()
        for f in FIELDS:
            getattr(m, f).flags.writeable = False
        _WITNESSES[depth] = m
    return _WITNESSES[depth]


def _state(led, c):
    values, present = led.accounts(c.indices)
    report = led.audit()
    return led.root().tobytes(), values.tobytes(), present.tobytes(), (report.consistent, report.n_bad, report.n_nodes)


@pytest.mark.parametrize("depth", [3, 15])
def test_messages_are_those_of_the_witness_the_batch_leaves(backend, depth):
    c = case(depth)
    w = _unsigned_witness(backend, depth)
    assert len(SC.nonce_moved(w)) >= 6, "the batch moves nonces inside itself"
    led = c.ledger(backend)
    before = _state(led, c)
    messages = led.messages(c.batch)
    assert messages.shape == (16, 28) and np.array_equal(messages, SC.tx_messages(w))
    assert _state(led, c) == before
    led.close()


@pytest.mark.parametrize("depth", [3, 15])
def test_signed_batch_is_applied_checked_and_proves(backend, depth):
    from certificate_stark_amd.prover import get_example_options
    c = case(depth)
    w = _unsigned_witness(backend, depth)
    led = c.ledger(backend)
    before = _state(led, c)
    signed = led.sign(c.batch, c.secrets, seed=SEED)
    assert _state(led, c) == before, "sign changed the ledger"
    s, r, d, rx, ss = signed
    assert np.array_equal(s, c.s) and np.array_equal(r, c.r) and np.array_equal(d, c.deltas)
    ref = SG.Signed(SC.tx_messages(w), c.secrets, SEED, 256)
    assert np.array_equal(rx, ref.sig_rx) and np.array_equal(ss, ref.sig_s)
    m = led.apply(signed, check_signatures=True)
    for f in FIELDS:
        expected = rx if f == "sig_rx" else ss if f == "sig_s" else getattr(w, f)
        assert np.array_equal(getattr(m, f), expected), f
    assert np.array_equal(led.root(), w.final_root)
    proof = backend.prove(get_example_options())
    assert int(backend.tx_verify([proof], m.initial_roots[0], m.final_root)[0]) == 0
    led.close()


@pytest.mark.parametrize("t,where,bit", [(0, "s", 0), (7, "s", 254), (15, "s", 255), (3, "rx", 0), (9, "rx", 5 * 64 + 17), (1, "s", 100)])
def test_a_flipped_bit_is_refused_at_its_transfer(backend, t, where, bit):
    from certificate_stark_amd.prover import Ledger, TransferRefused
    c = case(3)
    led = c.ledger(backend)
    s, r, d, rx, ss = led.sign(c.batch, c.secrets, seed=SEED)
    rx, ss = rx.copy(), ss.copy()
    if where == "s":
        ss[t, bit // 8] ^= 1 << (bit % 8)
    else:
        rx[t, bit // 64] ^= np.uint64(1 << (bit % 64))
        assert int(rx[t, bit // 64]) < SC.P
    with pytest.raises(TransferRefused) as e:
        led.apply((s, r, d, rx, ss), check_signatures=True)
    assert (e.value.index, e.value.reason) == (t, Ledger.SIGNATURE)
    led.close()


def _refusal(led, batch, secrets, call="sign"):
    from certificate_stark_amd.prover import TransferRefused
    with pytest.raises(TransferRefused) as e:
        if call == "sign":
            led.sign(batch, secrets, seed=SEED)
        elif call == "messages":
            led.messages(batch)
        else:
            led.apply(batch + (np.zeros((len(batch[0]), 6), np.uint64), np.zeros((len(batch[0]), 32), np.uint8)), want_witness=False)
    return e.value.index, e.value.reason


def test_sign_refuses_where_apply_refuses(backend):
    from certificate_stark_amd.backend import to_numpy_u64
    from certificate_stark_amd.prover import Ledger
    c = case(3)
    O = SC._oracle()
    led = c.ledger(backend)
    backend.upload_witness(_unsigned_witness(backend, 3))     # the witness that is resident while sign refuses and signs
    trace_before = to_numpy_u64(backend.build_trace()).copy()
    before = _state(led, c)
    absent = 2
    assert absent not in set(int(i) for i in c.indices)
    changes = {Ledger.INDEX_RANGE: ("s", 8), Ledger.SELF_TRANSFER: ("s", int(c.r[9])), Ledger.ABSENT: ("r", absent),
               Ledger.BALANCE: ("d", int(O.to_mont(np.array([1013], np.uint64))[0]))}      # transfer 9: one above what its sender holds by then
    for reason, (field, value) in changes.items():
        s, r, d = (a.copy() for a in c.batch)
        {"s": s, "r": r, "d": d}[field][9] = value
        for call in ("sign", "messages", "apply"):
            assert _refusal(led, (s, r, d), c.secrets, call) == (9, reason), (reason, call)
        # a wrong secret below the refusal comes first, one at or above it does not show
        wrong = c.secrets.copy()
        wrong[4] = 6
        wrong[6] = 1
        wrong[12] = 1
        assert _refusal(led, (s, r, d), wrong) == (4, Ledger.KEY)
        wrong = c.secrets.copy()
        wrong[9:] = 1 + wrong[9:] % 6
        assert _refusal(led, (s, r, d), wrong) == (9, reason)
        assert _state(led, c) == before
    # a wrong secret alone: KEY at the first one, and the text says so
    wrong = c.secrets.copy()
    wrong[5] = 1
    wrong[11] = 2
    assert _refusal(led, c.batch, wrong) == (5, Ledger.KEY) and Ledger.KEY == SG.KEY and "secret" in Ledger.REASONS[Ledger.KEY]
    assert _state(led, c) == before
    led.sign(c.batch, c.secrets, seed=SEED)
    assert _state(led, c) == before
    assert (backend.n_tx, backend.depth) == (16, 3)
    assert np.array_equal(to_numpy_u64(backend.build_trace()), trace_before), "sign changed the resident witness"
    led.close()


def test_sign_misuse_is_an_error(backend):
    from certificate_stark_amd import CstarkError
    c = case(3)
    led = c.ledger(backend)
    bad = c.secrets.copy()
    bad[3] = 0
    with pytest.raises(CstarkError) as e:
        led.sign(c.batch, bad, seed=SEED)
    assert e.value.code == -1 and "secrets[3]" in str(e.value)
    with pytest.raises(CstarkError) as e:
        led.sign(c.batch, c.secrets, seed=SEED, max_attempts=0)
    assert e.value.code == -1
    # an exhausted signature is an error that names the transfer
    ref = SG.Signed(SC.tx_messages(_unsigned_witness(backend, 3)), c.secrets, SEED, 1)
    first = int(np.flatnonzero(ref.status == SG.EXHAUSTED)[0])
    with pytest.raises(CstarkError) as e:
        led.sign(c.batch, c.secrets, seed=SEED, max_attempts=1)
    assert e.value.code == -5 and "transfer %d " % first in str(e.value)
    led.close()


@pytest.mark.parametrize("depth", [3, 15])
def test_a_partial_ledger_signs_the_same(backend, depth):
    from certificate_stark_amd.prover import Ledger
    c = case(depth)
    led = c.ledger(backend)
    signed = led.sign(c.batch, c.secrets, seed=SEED)
    part = led.open_multi_for(c.batch).to_ledger()
    assert part.partial
    root = part.root().copy()
    again = part.sign(c.batch, c.secrets, seed=SEED)
    for a, b in zip(signed, again):
        assert np.array_equal(a, b)
    assert np.array_equal(part.messages(c.batch), led.messages(c.batch))
    assert np.array_equal(part.root(), root)
    # an account the partial ledger does not know: UNKNOWN, from sign and from messages as from apply
    bystander = np.uint64(5 if depth == 3 else 9)
    led.set_accounts([bystander], c.values[:1])
    part2 = led.open_multi_for(c.batch).to_ledger()
    s, r, d = (a.copy() for a in c.batch)
    r[6] = bystander
    for call in ("sign", "messages", "apply"):
        assert _refusal(part2, (s, r, d), c.secrets, call) == (6, Ledger.UNKNOWN), call
    part.close()
    part2.close()
    led.close()
