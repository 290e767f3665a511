"""cstark::TransactionExample::verify and cstark::verify_batch (include/cstark.hpp), built with g++ like tests/cpp/host_mirror.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "verify_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "verify_mirror.cpp"),
                           "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_verify_mirror_compiles(tmp_path):
    assert os.path.exists(build_program(str(tmp_path)))


@pytest.mark.gpu
def test_verify_mirror_accepts_and_rejects(tmp_path):
    exe = build_program(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "accepted=1 rejected=5 batch=0,5" in res.stdout  # 5 = CSTARK_PROOF_REMAINDER_COMMITMENT
