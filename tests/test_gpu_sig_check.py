"""cstark_schnorr_check_signatures (Backend.schnorr_check) against the oracle's SchnorrAir trace (sig_cases.reference): verdicts and the
affine x of s*G + h*P bit for bit, on generated signatures at every size around the kernels' groupings (four hashes per wave, one wave
per ladder), on one-change perturbations, a key off the curve, the scalar extremes; refusals that launch nothing; a resident witness that
the check leaves alone.  Outputs start as 0xA5 and are compared whole."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC

pytestmark = pytest.mark.gpu

u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _check(backend, messages, sig_rx, sig_s, count=None, null=None):
    """the C call on 0xA5-filled outputs -> (status, verdicts, x)"""
    m, rx = np.ascontiguousarray(messages, np.uint64), np.ascontiguousarray(sig_rx, np.uint64)
    s = np.ascontiguousarray(sig_s, np.uint8)
    n = len(m) if count is None else count
    verdicts = np.full(max(len(m), 1), 0xA5, np.uint8)
    x = np.full((max(len(m), 1), 6), 0xA5A5A5A5A5A5A5A5, np.uint64)
    args = [m.ctypes.data_as(u64p), rx.ctypes.data_as(u64p), s.ctypes.data_as(u8p), verdicts.ctypes.data_as(u8p), x.ctypes.data_as(u64p)]
    if null is not None:
        args[null] = None
    rc = backend.lib.cstark_schnorr_check_signatures(backend.ctx, C.c_uint32(n), *args)
    return rc, verdicts, x


def _assert_reference(backend, arrays, expected=None):
    ref_v, ref_x = SC.reference(*arrays)
    if expected is not None:
        assert list(ref_v) == list(expected), "the reference itself disagrees with the case"
    rc, verdicts, x = _check(backend, *arrays)
    assert rc == 0, backend.lib.cstark_last_error()
    assert np.array_equal(verdicts, ref_v), (verdicts, ref_v)
    assert np.array_equal(x, ref_x)


# 1..5: partial and full groups of the hash kernel (four hashes per wave); 64, 65: many workgroups and a group of one behind them
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 7, 8, 9, 64, 65])
def test_generated_signatures_are_valid(backend, count):
    arrays = SC.generated(count)
    ref_v, ref_x = SC.generated_reference(count)
    assert not ref_v.any() and np.array_equal(ref_x, arrays[1])
    rc, verdicts, x = _check(backend, *arrays)
    assert rc == 0, backend.lib.cstark_last_error()
    assert np.array_equal(verdicts, np.zeros(count, np.uint8))
    assert np.array_equal(x, ref_x)


@pytest.mark.parametrize("j", [0, 7])
@pytest.mark.parametrize("kind", SC.PERTURBATIONS)
def test_one_change_is_a_mismatch_of_that_signature_alone(backend, kind, j):
    expected = [SC.VALID] * 8
    expected[j] = SC.MISMATCH
    _assert_reference(backend, SC.perturbed(SC.generated(8), j, kind), expected)


@pytest.mark.parametrize("j", [0, 5])
def test_key_off_the_curve(backend, oracle, j):
    arrays = SC.off_curve(SC.generated(8), j)
    assert oracle.lib().cso_ecc_on_curve_affine(oracle._p(np.ascontiguousarray(arrays[0][j, :12]))) == 0
    expected = [SC.VALID] * 8
    expected[j] = SC.KEY_NOT_ON_CURVE
    _assert_reference(backend, arrays, expected)


def test_scalar_extremes(backend):
    arrays = SC.scalar_extremes(SC.generated(8))
    _assert_reference(backend, arrays, [SC.MISMATCH] * 4 + [SC.SCALAR_RANGE])
    # the range verdict comes first: bit 255 set on a key off the curve and on a mismatch
    m, rx, s = SC.off_curve(arrays, 4)
    s[0, 31] |= 0x80
    _assert_reference(backend, (m, rx, s), [SC.SCALAR_RANGE] + [SC.MISMATCH] * 3 + [SC.SCALAR_RANGE])
    # and the key verdict before the mismatch
    m, rx, s = SC.off_curve(SC.perturbed(SC.generated(8), 1, "rx_word0"), 1)
    _assert_reference(backend, (m, rx, s), [0, SC.KEY_NOT_ON_CURVE, 0, 0, 0, 0, 0, 0])


def test_refusals_launch_nothing_and_leave_the_outputs(backend):
    m, rx, s = SC.generated(5)
    untouched_v, untouched_x = np.full(5, 0xA5, np.uint8), np.full((5, 6), 0xA5A5A5A5A5A5A5A5, np.uint64)

    def refused(*args, **kw):
        rc, verdicts, x = _check(backend, *args, **kw)
        assert rc == -1
        assert np.array_equal(verdicts, untouched_v) and np.array_equal(x, untouched_x)
        return backend.lib.cstark_last_error().decode()

    refused(m, rx, s, count=0)
    refused(m, rx, s, count=(1 << 20) + 1)
    for null in (0, 1, 2, 3):
        refused(m, rx, s, null=null)
    bad = m.copy()
    bad[2, 13] = SC.P
    bad[4, 0] = SC.P
    assert "messages[2][13]" in refused(bad, rx, s)
    bad = rx.copy()
    bad[3, 5] = SC.P
    assert "sig_rx[3][5]" in refused(m, bad, s)
    # a null rx_out is no refusal
    rc, verdicts, x = _check(backend, m, rx, s, null=4)
    assert rc == 0 and not verdicts.any() and np.array_equal(x, untouched_x)


def test_python_layers(backend):
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample
    m, rx, s = SC.perturbed(SC.generated(8), 3, "s_bit0")
    verdicts = backend.schnorr_check(m, rx, s)
    assert verdicts.dtype == np.uint8 and list(verdicts) == [0, 0, 0, backend.SIG_MISMATCH, 0, 0, 0, 0]
    verdicts2, x = backend.schnorr_check(m, rx, s, want_rx=True)
    assert np.array_equal(verdicts2, verdicts) and np.array_equal(x, SC.reference(m, rx, s)[1])
    with pytest.raises(ValueError):
        backend.schnorr_check(m, rx[:7], s)
    example = SchnorrExample(ProofOptions(), *(a.copy() for a in SC.generated(4)), backend=backend)
    assert list(example.check()) == [0, 0, 0, 0]


def test_resident_witness_is_not_touched(backend):
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample, get_example_options
    w = LC.generated((2, 3, 2))
    backend.upload_witness(w)
    before = backend.prove(get_example_options())
    assert not backend.schnorr_check(*SC.generated(5)).any()
    assert backend.prove(get_example_options()) == before
    # the same beside a resident SchnorrAir witness (its message tails and statement caches)
    example = SchnorrExample(ProofOptions(), *(a.copy() for a in SC.generated(2, seed=7)), backend=backend)
    before = example.prove()
    assert list(backend.schnorr_check(*SC.perturbed(SC.generated(5), 1, "msg26"))) == [0, SC.MISMATCH, 0, 0, 0]
    assert example.prove() == before
    example.verify(before)
