"""The composition stage at every blowup it serves: cstark_composition_columns against the oracle for log_blowup 1..6 -- 1..3 take
per-coset interpolations and k_coset_combine<1..3> (blowup 2 and 4: RangeProofAir, MerkleAir, RescueAir), 4..6 take interleave_cosets and
one transform of b n points -- at lengths from 2^6, where a workgroup of 256 threads is only partly filled.  Bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2**62 + 2**56 + 2**55 + 1
EXTREME_SHAPES = [(6, 1), (7, 2), (8, 3), (6, 4), (8, 6)]    # (log_n, log_blowup)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.mark.parametrize("log_n", [6, 7, 8, 11])
@pytest.mark.parametrize("log_blowup", [1, 2, 3, 4, 5, 6])
def test_composition_columns_at_every_blowup(oracle, backend, log_blowup, log_n):
    from certificate_stark_amd.backend import to_numpy_u64
    b, n = 1 << log_blowup, 1 << log_n
    rng = np.random.default_rng(100 * log_blowup + log_n)
    inputs = [("random", oracle.to_mont(rng.integers(0, P, size=b * n, dtype=np.uint64)))]
    if (log_n, log_blowup) in EXTREME_SHAPES:
        alt = np.zeros(b * n, np.uint64)
        alt[1::2] = P - 1
        inputs += [("all p - 1", np.full(b * n, P - 1, np.uint64)), ("alternating", alt)]
    for what, comb in inputs:
        comb = comb.reshape(b, n)
        ref = oracle.composition_columns(comb)
        got = to_numpy_u64(backend.composition_columns(backend.from_numpy_u64(comb)))
        assert got.shape == ref.shape == (b, n)
        assert (got == ref).all(), "%s: columns that differ: %s" % (what, sorted(set(np.argwhere(got != ref)[:, 0].tolist())))


@pytest.mark.parametrize("log_blowup", [1, 2, 4])
def test_interleave_cosets_is_the_transpose(backend, log_blowup):
    from certificate_stark_amd.backend import to_numpy_u64
    b, n = 1 << log_blowup, 64
    cm = np.arange(b * n, dtype=np.uint64).reshape(b, n) * np.uint64(0x9E3779B1) + np.uint64(7)
    got = to_numpy_u64(backend.interleave_cosets(backend.from_numpy_u64(cm)))
    assert (got == np.ascontiguousarray(cm.T).ravel()).all()


def test_composition_columns_refusals(backend):
    """through the C ABI: nothing is launched for a blowup, a length or a domain outside 2 <= b <= 64, 2^6 <= n, b n <= 2^24"""
    d_in, d_out = backend.from_numpy_u64(np.zeros(1 << 13, np.uint64)), backend.from_numpy_u64(np.full(1 << 13, 5, np.uint64))
    for log_n, log_blowup in [(6, 0), (6, 7), (5, 1), (19, 6), (24, 1)]:
        rc = backend.lib.cstark_composition_columns(backend.ctx, backend._ptr(d_in), backend._ptr(d_out), C.c_uint32(log_n), C.c_uint32(log_blowup))
        assert rc != 0, (log_n, log_blowup)
    backend.synchronize()
    assert (d_out.cpu().numpy() == 5).all()
    assert backend.lib.cstark_composition_columns(backend.ctx, backend._ptr(d_in), backend._ptr(d_out), C.c_uint32(6), C.c_uint32(1)) == 0
