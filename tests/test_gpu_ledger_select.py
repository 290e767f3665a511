"""Ledger.select (cstark_ledger_select) on the pools of select_cases.py at depth 3 and 7: seven accounts with secrets 1..7, pools of 12 to
25 candidates built by signing an appliable skeleton with Ledger.sign and splicing candidates in or corrupting signatures afterwards.
The reference is tests/select_model.py, whose signature verdicts come from Backend.schnorr_check on the model's OWN messages -- existing
code, tested apart -- so statuses, selection and messages are compared with a sequential walk that knows nothing of the product's
passes.  Then: chunk sizes, the read-only call, the applied selection against Ledger.apply on a twin, the unchecked call, misuse."""
import numpy as np
import pytest

import ledger_model as LM
import select_cases as SC
import select_model as SM

pytestmark = pytest.mark.gpu

SEED = 0x5E1EC7
FIELDS = ("initial_roots", "final_root", "s_old_values", "r_old_values", "s_indices", "r_indices", "s_paths", "r_paths", "deltas", "sig_rx", "sig_s")
CASES = [(name, depth) for name in SC.CASES for depth in SC.DEPTHS]


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


_KEYS, _SIGNED = {}, {}


def keys(backend):
    if "k" not in _KEYS:
        k = backend.schnorr_public_keys(np.arange(1, SC.N_ACC + 1, dtype=np.uint64))
        k.flags.writeable = False
        _KEYS["k"] = k
    return _KEYS["k"]


def clean_ledger(backend, pool):
    from certificate_stark_amd.prover import Ledger
    led = Ledger(pool.depth, backend)
    led.set_accounts(pool.indices(), pool.values(keys(backend)))
    return led


def signed_skeleton(backend, pool):
    """the skeleton's signatures, made once per (depth, skeleton) on a ledger of its own and shared, read-only"""
    key = (pool.depth, tuple(pool.skeleton))
    if key not in _SIGNED:
        led = clean_ledger(backend, pool)
        s, r, d, secrets = pool.skeleton_batch()
        _, _, _, rx, ss = led.sign((s, r, d), secrets, seed=SEED)
        led.close()
        rx.flags.writeable = False
        ss.flags.writeable = False
        _SIGNED[key] = (rx, ss)
    return _SIGNED[key]


class Setup:
    """a pool on the device: the ledger (a partial one where the pool asks for it), the five arrays, and the model of the same state"""

    def __init__(self, backend, pool):
        self.pool, self.backend = pool, backend
        values = pool.values(keys(backend))
        full = clean_ledger(backend, pool)
        if pool.off_curve is not None:
            values[pool.off_curve, 3] = (int(values[pool.off_curve, 3]) + 1) % SC.P
            full.set_accounts([pool.leaf(pool.off_curve)], values[pool.off_curve:pool.off_curve + 1])
        self.known = None
        if pool.partial:
            s, r, _, _ = pool.skeleton_batch()
            self.led = full.open_multi_for((s, r)).to_ledger()
            full.close()
            self.known = pool.known()
            assert self.led.partial
        else:
            self.led = full
        self.model = LM.LedgerModel(pool.depth)
        self.model.set_accounts(pool.indices(), values)
        self.rx, self.ss = pool.signatures(*signed_skeleton(backend, pool))
        self.transfers = pool.batch() + (self.rx, self.ss)
        self.device_verdicts = {}

    def sig_ok(self, t, message):
        v = int(self.backend.schnorr_check(message.reshape(1, 28), self.rx[t:t + 1], self.ss[t:t + 1])[0])
        self.device_verdicts[t] = v
        return v == 0

    def expected(self, check_signatures=True, want=None, pow2=None):
        s, r, d = self.pool.batch()
        return SM.select(self.model, s, r, d, self.pool.want if want is None else want, sig_ok=self.sig_ok if check_signatures else None,
                         sig_rx=self.rx, pow2=self.pool.pow2 if pow2 is None else pow2, known=self.known)

    def state(self):
        values, present = self.led.accounts(self.pool.indices() if self.known is None else self.known)      # a partial ledger: those it knows
        report = self.led.audit()
        return self.led.root().tobytes(), values.tobytes(), present.tobytes(), (report.consistent, report.n_bad, report.n_nodes)

    def close(self):
        self.led.close()


def with_verdict(pool, expected):
    """candidates whose status came from a device verdict: APPLIED, or SIGNATURE with a reduced sig_rx"""
    return [t for t in range(pool.n) if expected.status[t] == SM.APPLIED or (expected.status[t] == SM.SIGNATURE and pool.entries[t].sig != "rx_ge_p")]


@pytest.mark.parametrize("name,depth", CASES, ids=["%s-d%d" % c for c in CASES])
def test_select_gives_the_models_statuses_selection_and_messages(backend, name, depth):
    pool = SC.CASES[name](depth)
    u = Setup(backend, pool)
    exp = u.expected()
    SC.check_landmarks(name, exp.status)
    before = u.state()
    sel = u.led.select(u.transfers, pool.want, pow2=pool.pow2, want_messages=True)
    assert u.state() == before, "a select without apply changed the ledger"
    assert np.array_equal(sel.status, exp.status), (list(sel.status), list(exp.status))
    assert np.array_equal(sel.selected, exp.selected) and len(sel) == len(exp.selected)
    assert sel.counts == exp.counts and sum(sel.counts) == pool.n == sel.report.n_candidates and sel.report.n_selected == len(exp.selected)
    assert not np.array(sel.report.root_after, np.uint64).any() and sel.witness is None
    for t in with_verdict(pool, exp):
        assert np.array_equal(sel.messages[t], exp.messages[t]), t
    for t, e in enumerate(pool.entries):      # never sent to the device: statically refused, or sig_rx not reduced
        if e.sig == "rx_ge_p" or exp.status[t] in (SM.INDEX_RANGE, SM.SELF_TRANSFER, SM.ABSENT, SM.UNKNOWN):
            assert not sel.messages[t].any(), t
    for a, b in zip(sel.transfers, exp.transfers(u.transfers)):
        assert np.array_equal(a, b)
    if name == "all_valid":
        assert np.array_equal(sel.messages, u.led.messages(u.transfers)) and sel.report.n_chunks == 1 and sel.report.n_sig_checked == pool.n
        u.led.apply(u.transfers, want_witness=False, check_signatures=True)      # and the checked apply accepts exactly this
    if name == "off_curve_key":
        assert u.device_verdicts[2] == 2, "the sender's own candidate is refused for its key"
    u.close()


@pytest.mark.parametrize("chunk", [1, 3, 5])
def test_the_result_does_not_depend_on_the_chunk(backend, chunk):
    pool = SC.CASES["chunks_24"](7)
    u = Setup(backend, pool)
    exp = u.expected()
    whole = u.led.select(u.transfers, pool.want, pow2=False, want_messages=True)
    sel = u.led.select(u.transfers, pool.want, pow2=False, chunk=chunk, want_messages=True)
    assert np.array_equal(whole.status, exp.status) and np.array_equal(whole.selected, exp.selected)
    assert np.array_equal(sel.status, whole.status) and np.array_equal(sel.selected, whole.selected) and sel.counts == whole.counts
    needed = with_verdict(pool, exp)
    assert {0, 1} <= {sum(1 for e in pool.entries[:t] if e.s == pool.entries[t].s) and 1 for t in needed}, "k_t = 0 and k_t > 0 are both there"
    for t in needed:
        assert np.array_equal(sel.messages[t], exp.messages[t]) and np.array_equal(whole.messages[t], exp.messages[t]), t
    assert whole.report.n_chunks == 1 and sel.report.n_chunks > 1
    assert len(needed) <= sel.report.n_sig_checked <= whole.report.n_sig_checked <= pool.n
    if chunk == 1:
        assert sel.report.n_sig_checked == sel.report.n_chunks == len(needed)
    u.close()


def test_without_check_signatures_nothing_is_checked(backend):
    pool = SC.CASES["flipped_s"](3)
    u = Setup(backend, pool)
    exp = u.expected(check_signatures=False)
    assert SM.SIGNATURE not in exp.status
    for pool_transfers in (u.transfers, pool.batch()):      # with the signatures and without them
        sel = u.led.select(pool_transfers, pool.want, check_signatures=False, pow2=False, want_messages=True)
        assert np.array_equal(sel.status, exp.status) and np.array_equal(sel.selected, exp.selected)
        assert sel.report.n_sig_checked == 0 and sel.report.n_chunks == 0 and not sel.messages.any()
    u.close()


def test_select_is_read_only_and_leaves_the_resident_witness(backend):
    from certificate_stark_amd.prover import get_example_options
    pool = SC.CASES["all_valid"](3)
    u = Setup(backend, pool)
    two = tuple(a[:2] for a in u.transfers)
    twin = Setup(backend, pool)
    m = twin.led.apply(two, check_signatures=True)      # a resident 2-transfer witness
    proof = backend.prove(get_example_options())
    before = u.state()
    for name in ("all_valid", "flipped_s", "overdraft"):
        other = SC.CASES[name](3)
        rx, ss = other.signatures(*signed_skeleton(backend, other))
        u.led.select(other.batch() + (rx, ss), other.want, want_messages=True)
    assert u.state() == before
    assert (backend.n_tx, backend.depth) == (2, 3)
    assert backend.prove(get_example_options()) == proof, "a select changed the resident witness"
    assert int(backend.tx_verify([proof], m.initial_roots[0], m.final_root)[0]) == 0
    u.close()
    twin.close()


@pytest.mark.parametrize("name,depth,want", [("flipped_s", 3, 2), ("flipped_s", 7, 12), ("overdraft", 7, 8), ("unknown", 3, 4)])
def test_applied_selection_is_the_checked_apply_of_its_transfers(backend, name, depth, want):
    from certificate_stark_amd.prover import get_example_options
    pool = SC.CASES[name](depth)
    u, twin = Setup(backend, pool), Setup(backend, pool)
    exp = u.expected(want=want, pow2=True)
    cp = u.led.checkpoint()
    root_before = u.led.root().copy()
    sel = u.led.select(u.transfers, want, pow2=True, apply=True)
    assert np.array_equal(sel.status, exp.status) and np.array_equal(sel.selected, exp.selected) and len(sel) & (len(sel) - 1) == 0 and len(sel)
    assert (backend.n_tx, backend.depth) == (len(sel), depth)
    proof = backend.prove(get_example_options()) if len(sel) == 2 else None
    m = twin.led.apply(sel.transfers, check_signatures=True)      # the twin is not refused
    for f in FIELDS:
        assert np.array_equal(getattr(sel.witness, f), getattr(m, f)), f
    assert np.array_equal(u.led.root(), twin.led.root()) and np.array_equal(np.array(sel.report.root_after, np.uint64), m.final_root)
    w = u.model.apply(*exp.transfers(pool.batch()))
    assert np.array_equal(w.final_root, m.final_root) and np.array_equal(w.s_paths, m.s_paths)
    assert u.led.audit().consistent
    if proof is not None:
        assert backend.prove(get_example_options()) == proof, "the resident witness of select(apply) differs from that of apply"
        assert int(backend.tx_verify([proof], m.initial_roots[0], m.final_root)[0]) == 0
    u.led.revert(cp)
    assert np.array_equal(u.led.root(), root_before)
    u.close()
    twin.close()


def test_apply_with_nothing_selected_changes_nothing(backend):
    pool = SC.nothing_selectable(3)
    u = Setup(backend, pool)
    before = u.state()
    sel = u.led.select(u.transfers, 4, apply=True)
    bad = (0, 1, 2, 4, 5, 6, 8)
    assert list(sel.status) == [SM.SIGNATURE if t in bad else SM.HELD for t in range(12)] and len(sel) == 0 and sel.witness is None
    assert np.array_equal(sel.status, u.expected(want=4, pow2=True).status)
    assert u.state() == before and not np.array(sel.report.root_after, np.uint64).any()
    u.close()


def test_misuse_is_an_error_and_leaves_the_outputs(backend):
    import ctypes as C
    from certificate_stark_amd import CstarkError, _lib
    from certificate_stark_amd.backend import Backend
    pool = SC.CASES["all_valid"](3)
    u = Setup(backend, pool)
    s, r, d, rx, ss = u.transfers
    n = pool.n
    status, selected, messages = np.full(n, 0xAB, np.uint8), np.full(n, 0xABABABAB, np.uint32), np.full((n, 28), 0xAB, np.uint64)
    report = _lib.LedgerSelectionStruct()
    C.memset(C.byref(report), 0xAB, C.sizeof(report))
    other = Backend()
    lib, ptr = backend.lib, backend._hptr
    u32p = C.POINTER(C.c_uint32)

    def call(ctx=None, n_=n, s_=s, d_=d, rx_=rx, ss_=ss, want=n, flags=1, chunk=0, status_=status, report_=report):
        opt = lambda a, typ=_lib.u64p: None if a is None else ptr(a, typ)
        return lib.cstark_ledger_select(ctx or backend.ctx, u.led._led, C.c_uint32(n_), opt(s_), ptr(r), opt(d_), opt(rx_), opt(ss_, _lib.u8p), C.c_uint32(want),
                                        C.c_uint32(flags), C.c_uint32(chunk), opt(status_, _lib.u8p), selected.ctypes.data_as(u32p), ptr(messages),
                                        None if report_ is None else C.byref(report_), None)

    bad_delta = d.copy()
    bad_delta[7] = SC.P
    before = u.state()
    misuse = dict(n_zero=dict(n_=0), n_large=dict(n_=2**20 + 1), want_zero=dict(want=0), want_large=dict(want=2**20 + 1), flag=dict(flags=8),
                  chunk_large=dict(chunk=2**20 + 1), null_s=dict(s_=None), null_deltas=dict(d_=None), null_status=dict(status_=None),
                  null_report=dict(report_=None), null_rx_checked=dict(rx_=None), null_s_applied=dict(ss_=None, flags=4),
                  other_context=dict(ctx=other.ctx), delta=dict(d_=bad_delta))
    for what, args in misuse.items():
        assert call(**args) == -1, what
        if what == "delta":
            assert "deltas[7]" in lib.cstark_last_error().decode()
        assert (status == 0xAB).all() and (selected == 0xABABABAB).all() and (messages == 0xAB).all(), what
        assert bytes(report) == b"\xab" * C.sizeof(report), what
    assert u.state() == before
    assert call() == 0 and list(status) == [0] * n and report.n_selected == n      # the same call without a mistake
    other.close()
    u.close()
