"""cstark::Ledger::from_multiproof, known and partial_info (include/cstark.hpp): tests/cpp/ledger_partial_check.cpp, written against the
header and compiled with g++, builds a partial ledger from one multi-opening of case (2 transfers, depth 3, seed 2), applies the batch to
it and to the full ledger and compares the witnesses field for field and with the reference's; an unopened account is refused as
CSTARK_LEDGER_UNKNOWN (reason 6) at the transfer that names it, unopened indices throw, a changed opening gives no ledger."""
import os
import subprocess

import pytest

import ledger_cases as LC
import multiproof_cases as MC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "ledger_partial_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ledger_partial_check.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_partial_ledger_round_trip(tmp_path):
    exe = build_program(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout == "built=1 refused=1,6 unchanged=1 threw=4 same=1 as_reference=1 audit=1 tampered=1,%d\n" % MC.ROOT, res.stdout


def test_cpp_ledger_partial_check_compiles():
    """CPU check: the header's partial-ledger wrappers are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
