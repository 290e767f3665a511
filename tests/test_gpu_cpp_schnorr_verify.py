"""verify() of the C++ mirror's SchnorrExample (include/cstark.hpp): tests/cpp/schnorr_verify.cpp, compiled with g++ the way
test_gpu_cpp_sub_air_verify.py builds its program, proves and verifies SchnorrAir on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "schnorr_verify")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "schnorr_verify.cpp"),
                           "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_schnorr_example_verifies(tmp_path):
    res = subprocess.run([build_program(str(tmp_path))], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("verdict") == 6


def test_cpp_schnorr_program_compiles(tmp_path):
    assert os.path.exists(build_program(str(tmp_path)))
