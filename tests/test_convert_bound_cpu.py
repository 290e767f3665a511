"""CPU: cstark_proof_convert_bound (host only) on the CPU oracle's proofs and their compact forms (tests/compact_cases.py), the statuses
of the convert calls that need no device (null context, null arguments), and csrc/proof_layout.h's convert_proof on its own
(tests/cpp/proof_convert_check.cpp, g++).

The bound to the plain form is the exact plain length, from either form; to the compact form it is the plain length plus one count
word per tree, which holds the compact proof whatever its positions."""
import ctypes as C
import os
import subprocess

import pytest

import compact_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("tx",) + (o,) for o in CC.TX_OPTS] + [("range",) + (o,) for o in CC.RANGE_OPTS]
INVALID_ARG = -1


def case(kind, opts):
    return CC.tx_case(2, 3, opts) if kind == "tx" else CC.range_case(opts)


@pytest.mark.parametrize("kind,opts", CASES)
def test_bound_of_both_forms(oracle, kind, opts):
    from certificate_stark_amd.verify import convert_bound
    plain, positions = case(kind, opts)
    compact = CC.compact(plain, positions)
    trees = len(CC.walk(plain)[1])
    assert convert_bound(plain, "compact") == len(plain) + 4 * trees
    assert convert_bound(plain, "compact") >= len(compact)
    assert convert_bound(compact, "plain") == len(plain)
    assert convert_bound(plain, "plain") == len(plain)
    assert convert_bound(compact, "compact") == len(plain) + 4 * trees


def test_bound_refuses_what_does_not_parse(oracle):
    from certificate_stark_amd import _lib
    from certificate_stark_amd.verify import convert_bound
    lib = _lib.load()
    plain, positions = CC.range_case(CC.RANGE_OPTS[3])
    compact = CC.compact(plain, positions)
    for proof in (plain, compact):
        for cut in (0, 3, 51, len(proof) // 2, len(proof) - 1):
            with pytest.raises(ValueError):
                convert_bound(proof[:cut], "plain")
        with pytest.raises(ValueError):
            convert_bound(proof + b"\0", "compact")                   # one trailing byte
        with pytest.raises(ValueError):
            convert_bound(proof, "short")
        with pytest.raises(ValueError):
            convert_bound(proof, 2)
    with pytest.raises(ValueError):
        convert_bound(b"CSTX" + plain[4:], "compact")
    # the C statuses: null pointers, another form, a truncated proof
    buf = (C.c_uint8 * len(plain)).from_buffer_copy(plain)
    bound = C.c_size_t(77)
    assert lib.cstark_proof_convert_bound(None, len(plain), 1, C.byref(bound)) == INVALID_ARG
    assert lib.cstark_proof_convert_bound(buf, len(plain), 1, None) == INVALID_ARG
    assert lib.cstark_proof_convert_bound(buf, len(plain), 2, C.byref(bound)) == INVALID_ARG
    assert lib.cstark_proof_convert_bound(buf, len(plain) - 1, 1, C.byref(bound)) == INVALID_ARG
    assert b"does not parse" in lib.cstark_last_error()
    assert bound.value == 77                                          # untouched by every refusal
    assert lib.cstark_proof_convert_bound(buf, len(plain), 0, C.byref(bound)) == 0 and bound.value == len(plain)


def test_convert_calls_refuse_a_null_context():
    from certificate_stark_amd import _lib
    lib = _lib.load()
    v = (C.c_int32 * 1)(-7)
    for fn in (lib.cstark_tx_convert, lib.cstark_air_convert):
        assert fn(None, 1, None, None, None, None, None, 1, None, None, None, v) == INVALID_ARG
    assert lib.cstark_schnorr_convert(None, 1, None, None, None, None, 1, None, None, None, v) == INVALID_ARG
    assert v[0] == -7


def test_convert_proof_on_its_own(tmp_path):
    """tests/cpp/proof_convert_check.cpp: both writers round-trip to byte equality with sections taken from the other form's parsed
    layout; a short buffer is left untouched"""
    exe = str(tmp_path / "proof_convert_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "proof_convert_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok 162 shapes"), out.stdout + out.stderr
