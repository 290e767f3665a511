"""The reference of the trace-validation tests (validate_cases.py) pinned on the CPU: on TransactionAir its first violation is the one
oracle.tx_check_trace finds, clean traces give all-clean codes for every AIR, and the boundary lists accept the statement a trace was
built for.  tests/cpp/trace_check_check.cpp (a stand-alone program, built with AddressSanitizer and UBSan and run directly) exercises
csrc/trace_check.h's list builder and decoder at the extremes."""
import os
import subprocess

import numpy as np
import pytest

import validate_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TX_CELLS = VC.TX_CELLS


@pytest.fixture(scope="module")
def tx_clean(oracle, witness_d3):
    trace = oracle.tx_build_trace(witness_d3)
    ref = VC.reference(oracle, VC.TX, trace, 3)           # every frame, row by row
    return trace, ref


def test_clean_traces_give_clean_codes(oracle, witness_d3, tx_clean):
    trace, ref = tx_clean
    assert ref.step is None and ref.bad_cycles == 0 and (ref.codes == VC.CLEAN).all() and ref.codes.size == 2
    assert oracle.tx_check_trace(trace, 2, 3) == -1
    pub = np.concatenate([witness_d3.initial_roots[0], witness_d3.final_root])
    assert VC.boundary_reference(oracle, VC.TX, trace, pub) is None
    m = oracle.merkle_build_trace(witness_d3)
    r = VC.reference(oracle, VC.MERKLE, m, 3)
    assert r.step is None and (r.codes == VC.CLEAN).all() and VC.boundary_reference(oracle, VC.MERKLE, m, pub) is None
    w = oracle.SchnorrWitness.generate(2, seed=9)
    s = oracle.schnorr_build_trace(w)
    r = VC.reference(oracle, VC.SCHNORR, s, statement=w)
    assert r.step is None and r.codes.size == 2 and VC.boundary_reference(oracle, VC.SCHNORR, s, statement=w) is None
    g = oracle.range_build_trace(12345)
    r = VC.reference(oracle, VC.RANGE, g)
    assert r.step is None and r.codes.size == 1 and VC.boundary_reference(oracle, VC.RANGE, g, oracle.to_mont([12345])) is None
    seed = oracle.to_mont(np.arange(42, 49, dtype=np.uint64))
    c = oracle.rescue_chain_build_trace(seed, 2)
    r = VC.reference(oracle, VC.RESCUE, c)
    assert r.step is None and r.codes.size == 2 and VC.boundary_reference(oracle, VC.RESCUE, c, np.concatenate([seed, c[:7, -1]])) is None


@pytest.mark.parametrize("name", sorted(TX_CELLS))
def test_first_violation_is_the_one_tx_check_trace_finds(oracle, tx_clean, name):
    trace, _ = tx_clean
    col, row = TX_CELLS[name]
    bad = VC.bump(trace, [(col, row)])
    ref = VC.reference(oracle, VC.TX, bad, 3, clean_trace=trace)
    want = oracle.tx_check_trace(bad, 2, 3)
    print("%s: cell (%d, %d) -> step %s constraint %s, %d bad cycles; tx_check_trace %d" % (name, col, row, ref.step, ref.constraint, ref.bad_cycles, want))
    assert ref.step is not None and ref.step * 115 + ref.constraint == want   # tx_check_trace: the lowest step * 115 + constraint
    assert ref.step in (row - 1, row) and ref.frame_values[ref.constraint] != 0
    assert ref.codes[ref.step // 1024] == (ref.step % 1024) * 115 + ref.constraint


def test_neighbour_frames_suffice(oracle, tx_clean):
    """tx_reference evaluates only the frames next to a changed row: the same codes as every frame evaluated"""
    trace, _ = tx_clean
    bad = VC.bump(trace, [(60, 100), (70, 1500)])
    a, b = VC.reference(oracle, VC.TX, bad, 3, clean_trace=trace), VC.reference(oracle, VC.TX, bad, 3)
    assert (a.codes == b.codes).all() and a.step == b.step and a.bad_cycles == b.bad_cycles == 2


def test_boundary_reference_names_the_altered_word(oracle, witness_d3, tx_clean):
    trace, _ = tx_clean
    pub = np.concatenate([witness_d3.initial_roots[0], witness_d3.final_root])
    for k in range(14):
        p = VC.bump(pub.reshape(1, 14), [(0, k)])[0]
        assert VC.boundary_reference(oracle, VC.TX, trace, p) == (k, 58 + k % 7, 0 if k < 7 else 2047)


def test_trace_check_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "trace_check_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "trace_check_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["ok: " + a for a in ("TransactionAir", "MerkleAir", "SchnorrAir", "RangeProofAir", "RescueAir",
                                                             "SchnorrAir, 1 signatures", "SchnorrAir, 4096 signatures")], out.stdout
