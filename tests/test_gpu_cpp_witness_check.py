"""cstark::check_witness and cstark::check_resident_witness (include/cstark.hpp): tests/cpp/witness_check_mirror.cpp, written against the
header and compiled with g++, checks honest and mutated small witnesses of witness_check_cases.py, signatures included; verdicts, folds,
report and final root are the plain model's, and a loaded witness checked where it lies gives what the host form gives."""
import os
import re
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import witness_check_cases as WC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "witness_check_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "witness_check_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def cases():
    """[(witness, Expected)]: honest witnesses of 1, 3 and 8 transfers, then every mutation of the depth-3 set and four of the depth-31 set"""
    honest = [WC.generated(1, 15), WC.generated(3, 1), WC.generated(8, 3), WC.generated(2, 31)]
    out = [(w, WC.check(w, check_signatures=True)) for w in honest]
    out += [(m, e) for _, m, e in WC.mutation_set(3)]
    out += [(m, e) for name, m, e in WC.mutation_set(31) if name in ("s_last_sibling", "r_index_top_bit", "delta_balance_plus_1", "sig_s_byte")]
    return out


def write_cases(path, witnesses):
    with open(path, "wb") as f:
        f.write(np.array([len(witnesses)], "<u8").tobytes())
        for w in witnesses:
            f.write(np.array([w.depth, w.n_tx], "<u8").tobytes())
            for name in w.FIELDS:
                f.write(np.ascontiguousarray(getattr(w, name), np.uint8 if name == "sig_s" else "<u8").tobytes())


@pytest.mark.gpu
def test_cpp_witness_check_follows_the_model(tmp_path):
    exe = build_program(str(tmp_path))
    todo = cases()
    assert set(int(v) for _, e in todo for v in e.verdicts) == set(range(10))
    write_cases(str(tmp_path / "cases"), [w for w, _ in todo])
    res = subprocess.run([exe, str(tmp_path / "cases"), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = re.match(r"witnesses=(\d+) resident=(\d+) same=(\d+)\n", res.stdout)
    assert got, res.stdout
    n_resident = sum(1 for w, _ in todo if w.n_tx & (w.n_tx - 1) == 0)
    assert [int(g) for g in got.groups()] == [len(todo), n_resident, n_resident] and n_resident >= 3
    words = np.fromfile(str(tmp_path / "out"), "<u8")
    at = 0
    for k, (w, e) in enumerate(todo):
        n = w.n_tx
        head, root = words[at:at + 5], words[at + 5:at + 12]
        verdicts, folds = words[at + 12:at + 12 + n], words[at + 12 + n:at + 12 + 29 * n].reshape(n, 4, 7)
        at += 12 + 29 * n
        assert list(head) == [n, w.depth, e.first_bad % 2**64, e.first_verdict, e.n_bad], k
        assert np.array_equal(root, e.final_root) and list(verdicts) == list(e.verdicts) and np.array_equal(folds, e.folds), k
    assert at == len(words)


def test_cpp_witness_check_mirror_compiles():
    """CPU check: the header's witness-check types are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
