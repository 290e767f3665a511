"""Conversion between the proof forms through the C++ mirror (include/cstark.hpp): tests/cpp/convert_mirror.cpp, compiled with g++ the
way test_gpu_cpp_compact.py builds its program, proves MerkleAir, RangeProofAir, RescueAir and SchnorrAir statements in both forms on
one context, converts each proof to the other form on the GPU and compares the bytes with the prover's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "convert_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "convert_mirror.cpp"),
                           "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_proofs_convert_both_ways(tmp_path):
    res = subprocess.run([build_program(str(tmp_path))], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("expected") == 23


def test_cpp_convert_program_compiles(tmp_path):
    assert os.path.exists(build_program(str(tmp_path)))
