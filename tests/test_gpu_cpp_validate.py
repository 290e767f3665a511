"""cstark::TraceReport, cstark::validate_trace and validate() of the five example classes (include/cstark.hpp):
tests/cpp/validate_mirror.cpp, written against the header and compiled with g++, validates per AIR the example's honest witness and
the same trace with one cell raised by 1.  The honest traces are the oracle's, the reports of the corrupted ones the reference's of
validate_cases.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import validate_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "certificate-stark_amd")
CELLS = {VC.TX: (60, 100), VC.MERKLE: (60, 512), VC.SCHNORR: (7, 511), VC.RANGE: (0, 7), VC.RESCUE: (3, 8)}


def build_program(tmp):
    exe = os.path.join(tmp, "validate_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "validate_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_reports_follow_the_reference(oracle, witness_d3, tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 5, res.stdout
    w = oracle.SchnorrWitness(2)
    w.messages[...] = np.fromfile(prefix + ".2.messages", np.uint64).reshape(2, 28)
    w.sig_rx[...] = np.fromfile(prefix + ".2.rx", np.uint64).reshape(2, 6)
    honest = {VC.TX: oracle.tx_build_trace(witness_d3), VC.MERKLE: oracle.merkle_build_trace(witness_d3), VC.SCHNORR: None,
              VC.RANGE: oracle.range_build_trace(12345),
              VC.RESCUE: oracle.rescue_chain_build_trace(oracle.to_mont(np.arange(42, 49, dtype=np.uint64)), 16)}
    units = {VC.TX: "transfer", VC.MERKLE: "transfer", VC.SCHNORR: "signature", VC.RANGE: "trace", VC.RESCUE: "link"}
    for air, text in enumerate(lines):
        got = re.fullmatch(r"air=(\d) clean=clean ok=1 \| (-?\d+) (\d+) (\d+) (-?\d+) \| (.*)", text)
        assert got and int(got.group(1)) == air, text
        trace = np.fromfile("%s.%d.trace" % (prefix, air), np.uint64).reshape(VC.WIDTH[air], -1)
        if honest[air] is not None:
            assert np.array_equal(trace, honest[air]), "air %d: the example's trace is not the oracle's" % air
        bad = VC.bump(trace, [CELLS[air]])
        if air == VC.TX:
            assert oracle.tx_check_trace(trace, 2, 3) == -1
        ref = VC.reference(oracle, air, bad, 3, statement=w, clean_trace=trace if air == VC.TX else None)
        step, constraint, bad_cycles, boundary = (int(got.group(k)) for k in (2, 3, 4, 5))
        assert (step, constraint, bad_cycles, boundary) == (ref.step, ref.constraint, ref.bad_cycles, -1), text
        assert np.array_equal(np.fromfile("%s.%d.codes" % (prefix, air), np.uint32), ref.codes)
        assert np.array_equal(np.fromfile("%s.%d.frame" % (prefix, air), np.uint64), ref.frame_values)
        cyc = VC.CYCLE[air] or trace.shape[1]
        assert got.group(6) == "%s %d, row %d, constraint %d" % (units[air], step // cyc, step % cyc, constraint), text


def test_cpp_validate_mirror_compiles():
    """CPU check: the header's validation types are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
