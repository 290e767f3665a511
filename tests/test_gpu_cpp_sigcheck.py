"""cstark::schnorr_check and Ledger::apply_checked (include/cstark.hpp): tests/cpp/sig_check_mirror.cpp, written against the header and
compiled with g++, checks generated and tampered signatures, is refused a batch with a forged signature and applies the batch as signed.
The x it reports for the tampered signature is the oracle trace's, its final root the oracle generator's."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "sig_check_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sig_check_mirror.cpp"),
                           "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_checked_apply_and_signature_check(tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "check=1 refused=1 witness_same=1" in res.stdout
    assert np.array_equal(np.fromfile(prefix + ".root", np.uint64), LC.generated((16, 3, 3)).final_root)
    _, x = SC.reference(*SC.perturbed(SC.generated(5), 3, "s_bit0"))
    assert np.array_equal(np.fromfile(prefix + ".rx", np.uint64), x[3])


def test_cpp_sig_check_mirror_compiles():
    """CPU check: the header's schnorr_check and Ledger::apply_checked are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
