"""GPU parity of the curve ladders (k_trace_schnorr_ec) on chosen scalars.

The ladder programs carry W = b3*Z as a fourth coordinate, so that a doubling and a mixed addition take two product phases each
(csrc/trace_gen.hip).  The trace must stay the reference's bit for bit: registers 0..36 (the ladder s*G, the bit register 18, the
ladder h*P) against the CPU oracle, for scalars that exercise doubling after doubling, doubling after addition, and the identity
(0 : 1 : 0, W = 0) through the complete formulas."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 2**255 - 1  # the ladder consumes bits 254..0
SCALARS = {
    "zero": 0,                                                    # doublings only: the point stays (0 : 1 : 0) and W stays 0
    "one": 1,                                                     # the identity doubled 255 times, then one addition to it
    "top_bit": 2**254,                                            # one addition to the identity, then doublings only
    "all_ones": MASK,                                             # an addition after every doubling
    "0x55": int.from_bytes(b"\x55" * 32, "little") & MASK,
    "0xaa": int.from_bytes(b"\xaa" * 32, "little") & MASK,
    "random": int.from_bytes(np.random.default_rng(0x1ADDE2).bytes(32), "little") & MASK,
}


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def golden(oracle):
    return oracle.TxWitness.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))


def _sub_witness(oracle, w, t0, cnt):
    s = oracle.TxWitness(cnt, w.depth)
    for f in s.FIELDS:
        if f != "final_root":
            getattr(s, f)[...] = getattr(w, f)[t0:t0 + cnt]
    s.final_root[...] = w.initial_roots[t0 + cnt]
    return s


def _scalar_bytes(s):
    return np.frombuffer(s.to_bytes(32, "little"), np.uint8)


def _report(got, ref, names):
    if not (got == ref).all():
        bad = np.argwhere(got != ref)
        c, r = bad[0]
        raise AssertionError("scalars %s: %d cells differ, registers %s, first at (register %d, row %d): got %x want %x" % (
            names, len(bad), sorted(set(bad[:, 0].tolist())), c, r, got[c, r], ref[c, r]))


# eight ladders (four transactions) are resident per CU: 7 transactions are no multiple of that, and take every scalar once
@pytest.mark.parametrize("names", [("zero", "one", "top_bit", "all_ones"), ("0x55", "0xaa", "random", "zero"), tuple(SCALARS)],
                         ids=["extremes", "alternating", "seven_transactions"])
def test_transaction_trace_ladders(oracle, backend, golden, names):
    from certificate_stark_amd.backend import to_numpy_u64
    w = _sub_witness(oracle, golden, 0, len(names))
    for t, name in enumerate(names):
        w.sig_s[t] = _scalar_bytes(SCALARS[name])
    ref = oracle.tx_build_trace(w)
    backend.upload_witness(w)
    got = to_numpy_u64(backend.build_trace())
    _report(got[:37], ref[:37], names)
    # the zero scalar never leaves the identity: X = Z = 0 on every ladder row (the last row of the block is the final addition's)
    for t, name in enumerate(names):
        if name == "zero":
            rows = slice(1024 * t + 512, 1024 * t + 512 + 511)
            assert not got[0:6, rows].any() and not got[12:18, rows].any()


@pytest.mark.parametrize("names", [("zero", "zero", "zero"), ("random", "all_ones", "one")], ids=["zero", "random"])
def test_schnorr_air_trace_ladders(oracle, backend, names):
    """the same ladders through the stand-alone SchnorrAir trace (512 rows per signature); three signatures"""
    from certificate_stark_amd.backend import to_numpy_u64
    w = oracle.SchnorrWitness.generate(len(names), seed=0x5C0)
    for t, name in enumerate(names):
        w.sig_s[t] = _scalar_bytes(SCALARS[name])
    ref = oracle.schnorr_build_trace(w)
    backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s)
    got = to_numpy_u64(backend.schnorr_build_trace())
    _report(got[:37], ref[:37], names)
