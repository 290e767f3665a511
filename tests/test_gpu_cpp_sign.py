"""cstark::schnorr_public_keys, schnorr_sign, schnorr_sign_nonces, Ledger::messages and Ledger::sign (include/cstark.hpp):
tests/cpp/sign_mirror.cpp, written against the header and compiled with g++, recovers the secrets of a generated batch from the public
keys, signs the batch through the ledger, is refused a wrong secret and applies the batch as signed.  What it writes is compared here
with the reference signer of sign_cases.py and the oracle generator's witness."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC
import sign_cases as SG

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "sign_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sign_mirror.cpp"),
                           "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_signs_a_batch_through_the_ledger(tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "recovered=1 key_refused=1 same_signer=1 valid=1 applied=1" in res.stdout
    w = LC.generated((16, 3, 3))
    assert np.array_equal(np.fromfile(prefix + ".root", np.uint64), w.final_root)
    assert np.array_equal(np.fromfile(prefix + ".keys", np.uint64).reshape(8, 12), SG.public_keys(range(1, 9)))
    secrets = np.fromfile(prefix + ".secrets", np.uint64)
    assert np.array_equal(SG.public_keys(secrets), w.s_old_values[:, :12])
    messages = np.fromfile(prefix + ".msg", np.uint64).reshape(16, 28)
    assert np.array_equal(messages, SC.tx_messages(w))
    ref = SG.Signed(messages, secrets, 11, 256)
    assert np.array_equal(np.fromfile(prefix + ".rx", np.uint64).reshape(16, 6), ref.sig_rx)
    assert np.array_equal(np.fromfile(prefix + ".s", np.uint8).reshape(16, 32), ref.sig_s)
    assert np.array_equal(np.fromfile(prefix + ".attempts", np.uint32), ref.attempts)
    rx, s, status = SG.attempts(messages[:3], secrets[:3], [0, 1, 2**255])
    assert np.array_equal(np.fromfile(prefix + ".nonce_rx", np.uint64).reshape(3, 6), rx)
    assert np.array_equal(np.fromfile(prefix + ".nonce_s", np.uint8).reshape(3, 32), s)
    assert np.array_equal(np.fromfile(prefix + ".nonce_status", np.uint8), status) and status[0] == SG.INFINITY


def test_cpp_sign_mirror_compiles():
    """CPU check: the header's signing calls are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
