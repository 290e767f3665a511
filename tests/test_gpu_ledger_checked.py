"""Ledger.apply(check_signatures=True) (cstark_ledger_apply_checked): a batch whose signatures are valid is applied exactly as the
unchecked call applies it (the oracle generator's eleven arrays, root and accounts); a bad signature refuses the batch with reason
SIGNATURE and changes nothing; the four older reasons keep their order ahead of it; the unchecked call accepts forged signatures as
it always did."""
import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC

pytestmark = pytest.mark.gpu

FIELDS = ("initial_roots", "s_old_values", "r_old_values", "s_indices", "r_indices", "s_paths", "r_paths", "deltas", "sig_rx", "sig_s")


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _ledger(backend, w):
    from certificate_stark_amd.prover import Ledger
    indices, initial = LC.initial_accounts(w)
    led = Ledger(w.depth, backend)
    led.set_accounts(indices, initial)
    return led, indices, initial


def _assert_applied(led, m, w, indices):
    for f in FIELDS:
        assert np.array_equal(getattr(m, f), getattr(w, f)), f
    assert np.array_equal(m.final_root, w.final_root) and np.array_equal(led.root(), w.final_root)
    values, present = led.accounts(indices)
    assert present.all() and np.array_equal(values, LC.final_accounts(w, indices))


def _checked_parity(backend, w):
    led, indices, _ = _ledger(backend, w)
    m = led.apply(SC.transfers(w), check_signatures=True)
    _assert_applied(led, m, w, indices)
    led.close()


@pytest.mark.parametrize("case", [(1, 3, 1), (16, 3, 3), (32, 3, 9), (4, 31, 6)], ids=LC.case_id)
def test_checked_apply_reproduces_the_generator(backend, case):
    w = LC.generated(case)
    if case[0] >= 16:
        # senders that sign a nonce an earlier transfer of the same batch moved: the message is built from the state before the
        # TRANSFER, not before the batch
        assert set({16: [4, 5, 6, 8], 32: [2, 4, 5]}[case[0]]) <= set(SC.nonce_moved(w))
    _checked_parity(backend, w)


def test_checked_apply_reproduces_the_committed_1024_transfer_witness(backend):
    _checked_parity(backend, LC.golden_1024())


@pytest.mark.parametrize("j", [0, 7, 15])
def test_a_bad_signature_refuses_and_changes_nothing(backend, j):
    from certificate_stark_amd.backend import to_numpy_u64
    from certificate_stark_amd.prover import Ledger, TransferRefused
    w = LC.generated((16, 3, 3))
    led, indices, initial = _ledger(backend, w)
    backend.upload_witness(LC.generated((2, 3, 2)))     # the witness that is resident when the refused batch arrives
    trace_before = to_numpy_u64(backend.build_trace()).copy()
    with pytest.raises(TransferRefused) as e:
        led.apply(SC.flipped(w, j), check_signatures=True)
    assert (e.value.index, e.value.reason) == (j, Ledger.SIGNATURE) and Ledger.SIGNATURE == SC.SIGNATURE
    assert "signature" in str(e.value)
    assert np.array_equal(led.root(), w.initial_roots[0])
    values, present = led.accounts(indices)
    assert present.all() and np.array_equal(values, initial)
    assert (backend.n_tx, backend.depth) == (2, 3)
    assert np.array_equal(to_numpy_u64(backend.build_trace()), trace_before), "a refused batch changed the resident witness"
    m = led.apply(SC.transfers(w), check_signatures=True)
    _assert_applied(led, m, w, indices)
    led.close()


def test_older_reasons_keep_their_order(backend, oracle):
    from certificate_stark_amd.prover import Ledger, TransferRefused
    w = LC.generated((16, 3, 3))
    led, indices, initial = _ledger(backend, w)

    def refusal(bad_signature=None):
        s, r, d, rx, ss = (a.copy() for a in SC.transfers(w))
        d[9] = oracle.to_mont(np.array([SC.P - 1], np.uint64))[0]   # above every balance; also breaks transfer 9's own signature
        if bad_signature is not None:
            ss[bad_signature, 0] ^= 1
        with pytest.raises(TransferRefused) as e:
            led.apply((s, r, d, rx, ss), check_signatures=True)
        assert np.array_equal(led.root(), w.initial_roots[0])
        return e.value.index, e.value.reason

    assert refusal() == (9, Ledger.BALANCE)
    assert refusal(3) == (3, Ledger.SIGNATURE)
    assert refusal(12) == (9, Ledger.BALANCE)
    values, _ = led.accounts(indices)
    assert np.array_equal(values, initial)
    led.close()


def test_unchecked_apply_accepts_a_forged_signature_as_before(backend):
    w = LC.generated((16, 3, 3))
    led, indices, _ = _ledger(backend, w)
    forged = SC.flipped(w, 7)
    m = led.apply(forged)
    assert np.array_equal(m.sig_s, forged[4]) and not np.array_equal(m.sig_s, w.sig_s)
    assert np.array_equal(m.final_root, w.final_root) and np.array_equal(led.root(), w.final_root)
    led.close()
