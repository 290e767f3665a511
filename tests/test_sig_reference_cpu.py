"""The references of the signature-check tests (sig_cases.py) against the oracle itself, no GPU: generated signatures are valid under
the reference and every perturbation the GPU tests use is invalid; the tx-message builder reproduces the message that the
TransactionAir trace hashes."""
import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC


@pytest.mark.parametrize("count", [1, 5, 8])
def test_generated_signatures_are_valid(count):
    verdicts, x = SC.generated_reference(count)
    assert not verdicts.any()
    assert np.array_equal(x, SC.generated(count)[1])


@pytest.mark.parametrize("j", [0, 7])
@pytest.mark.parametrize("kind", SC.PERTURBATIONS)
def test_every_perturbation_is_a_mismatch(kind, j):
    verdicts, x = SC.reference(*SC.perturbed(SC.generated(8), j, kind))
    expected = np.zeros(8, np.uint8)
    expected[j] = SC.MISMATCH
    assert np.array_equal(verdicts, expected)
    others = np.arange(8) != j
    assert np.array_equal(x[others], SC.generated(8)[1][others])


def test_key_off_the_curve_and_scalar_extremes(oracle):
    m, rx, s = SC.off_curve(SC.generated(8), 2)
    assert oracle.lib().cso_ecc_on_curve_affine(oracle._p(np.ascontiguousarray(m[2, :12]))) == 0
    verdicts, _ = SC.reference(m, rx, s)
    assert list(verdicts) == [0, 0, SC.KEY_NOT_ON_CURVE, 0, 0, 0, 0, 0]
    m, rx, s = SC.scalar_extremes(SC.generated(8))
    verdicts, x = SC.reference(m, rx, s)
    assert list(verdicts) == [SC.MISMATCH] * 4 + [SC.SCALAR_RANGE]
    assert np.array_equal(x[4], rx[4]), "bit 255 of s is not read by the trace"
    assert x[0].any(), "s = 0 leaves h*P, a finite point"


def test_tx_message_builder_reproduces_the_hashed_message(oracle):
    w = LC.generated((16, 3, 3))
    messages = SC.tx_messages(w)
    # the walk's state before every transfer is the witness's old values
    assert np.array_equal(messages[:, 0:12], w.s_old_values[:, :12]) and np.array_equal(messages[:, 12:24], w.r_old_values[:, :12])
    assert np.array_equal(messages[:, 24], w.deltas) and np.array_equal(messages[:, 25], w.s_old_values[:, 13])
    assert not messages[:, 26:].any()
    verdicts, x = SC.reference(messages, w.sig_rx, w.sig_s)
    assert not verdicts.any() and np.array_equal(x, w.sig_rx)
    # and it is the message the TransactionAir trace hashes: the x of row 1023 of every transfer is the same value
    trace = oracle.tx_build_trace(w)
    assert np.array_equal(np.ascontiguousarray(trace[0:6, 1023::1024].T), w.sig_rx)


@pytest.mark.parametrize("case,some", [((16, 3, 3), [4, 5, 6, 8]), ((32, 3, 9), [2, 4, 5])])
def test_cases_sign_nonces_that_moved_within_the_batch(case, some):
    moved = SC.nonce_moved(LC.generated(case))
    assert set(some) <= set(moved), moved
