"""cstark::Ledger (include/cstark.hpp): tests/cpp/ledger_mirror.cpp, written against it and compiled with g++, puts the accounts of
case (2 transfers, depth 3, seed 2) into a ledger, applies the transfers and proves the resident batch without an upload.  Its final
root is the oracle generator's, its proof the bytes of the uploaded oracle witness."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "ledger_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ledger_mirror.cpp"),
                           "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_ledger_reproduces_root_and_proof(tmp_path):
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import get_example_options
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "root_before=1 refused=1 witness_same=1" in res.stdout
    w = LC.generated((2, 3, 2))
    assert np.array_equal(np.fromfile(prefix + ".root", np.uint64), w.final_root)
    b = Backend()
    b.upload_witness(w)
    assert open(prefix + ".proof", "rb").read() == b.prove(get_example_options())
    b.close()


def test_cpp_ledger_mirror_compiles():
    """CPU check: the header's Ledger is self-contained C++17 and links against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
