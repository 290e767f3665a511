"""cstark::Ledger::select (include/cstark.hpp): tests/cpp/ledger_select_mirror.cpp, written against it and compiled with g++, signs the
batch of build_random(16, depth 3, seed 3), flips a scalar bit of candidate 5, splices a self transfer in at 9 and selects: read-only
at two chunk sizes, then applied against apply_checked on a twin.  Statuses, selection, messages and the root are those of
tests/select_model.py on the pool the program wrote, with the model's signature verdicts from Backend.schnorr_check."""
import os
import subprocess

import numpy as np
import pytest

import ledger_model as LM
import select_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "ledger_select_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ledger_select_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_select_gives_the_models_selection(tmp_path):
    from certificate_stark_amd.backend import Backend
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "n=17 " in res.stdout and "read_only=1 chunk_free=1 same=1" in res.stdout, res.stdout
    load = lambda ext, dtype=np.uint64: np.fromfile(prefix + ext, dtype)
    idx, val = load(".idx"), load(".val").reshape(-1, 14)
    s, r, d, rx, ss = load(".s"), load(".r"), load(".d"), load(".rx").reshape(-1, 6), load(".ss", np.uint8).reshape(-1, 32)
    model = LM.LedgerModel(3)
    model.set_accounts(idx, val)
    b = Backend()
    sig_ok = lambda t, m: int(b.schnorr_check(m.reshape(1, 28), rx[t:t + 1], ss[t:t + 1])[0]) == 0
    exp = SM.select(model, s, r, d, 16, sig_ok=sig_ok, sig_rx=rx)
    cut = SM.select(model, s, r, d, 16, sig_ok=sig_ok, sig_rx=rx, pow2=True)
    b.close()
    status = load(".status", np.uint8)
    assert np.array_equal(status, exp.status), (list(status), list(exp.status))
    assert status[5] == SM.SIGNATURE and status[9] == SM.SELF_TRANSFER and SM.HELD in status
    assert np.array_equal(load(".selected", np.uint32), exp.selected)
    messages = load(".msg").reshape(-1, 28)
    for t in exp.selected:
        assert np.array_equal(messages[t], exp.messages[int(t)]), t
    assert np.array_equal(load(".applied", np.uint32), cut.selected) and len(cut.selected) in (4, 8)
    w = model.apply(*cut.transfers((s, r, d)))
    assert np.array_equal(load(".root"), w.final_root)


def test_cpp_select_mirror_compiles():
    """CPU check: the header's Ledger::select is self-contained C++17 and links against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
