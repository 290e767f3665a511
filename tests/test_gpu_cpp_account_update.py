"""cstark::check_account_update (include/cstark.hpp): tests/cpp/account_update_mirror.cpp, written against the header and compiled with
g++, opens the accounts of case (2 transfers, depth 3, seed 2) and one absent index with one multiproof, lets the ledger move on and
checks the transition without the ledger: stated, compute-only, against a stale root, and with a node dropped.  The new root is the plain
model's, the verdicts and the changed count the plain folds' (update_cases.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import multiproof_cases as MC
import update_cases as UC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "account_update_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "account_update_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_update_check_follows_the_reference(tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = re.match(r"opened=1 n_nodes=(\d+) stated=(\d+),(\d+),(\d+),(\d) computed=(\d+),(\d+),(\d) stale=(\d+),(\d+),(\d) dropped=(\d+),(\d+)\n", res.stdout)
    assert got, res.stdout
    numbers = [int(g) for g in got.groups()]
    n_nodes, stated, computed, stale, dropped = numbers[0], numbers[1:5], numbers[5:8], numbers[8:11], numbers[11:]
    w = LC.generated((2, 3, 2))
    have, values = LC.initial_accounts(w)
    old = LM.LedgerModel(3)
    old.set_accounts(have, values)
    indices = np.fromfile(prefix + ".indices", np.uint64)
    assert len(indices) == len(have) + 1 and MC.first_bad_index(3, indices) is None
    new_values = np.fromfile(prefix + ".new_values", np.uint64).reshape(-1, 14)
    new_present = np.array([int(i) in old.value or v.any() for i, v in zip(indices, new_values)], np.uint8)
    new = old.copy()
    new.set_accounts([int(i) for i, p in zip(indices, new_present) if p], new_values[new_present.astype(bool)])
    new_root = np.fromfile(prefix + ".new_root", np.uint64)
    assert np.array_equal(new_root, new.root()) and not np.array_equal(new_root, old.root())
    old_values, old_present, _, _, nodes, old_root, _ = UC.states(old, new, indices)
    assert n_nodes == len(nodes)
    ref = UC.expected_update(3, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root)
    assert ref[:2] == (UC.VALID, 0) and ref[3] >= 1 and np.array_equal(ref[2], new_root)
    assert stated == [UC.VALID, 0, ref[3], 1] and computed == [UC.VALID, ref[3], 1]
    assert np.array_equal(np.fromfile(prefix + ".computed", np.uint64), new_root)
    assert stale == [UC.NEW_ROOT, ref[3], 1]
    assert dropped == list(UC.expected_update(3, indices, old_values, old_present, new_values, new_present, nodes[:-1], old_root, new_root)[:2])
    assert dropped == [UC.NODE_COUNT, n_nodes]


def test_cpp_account_update_mirror_compiles():
    """CPU check: the header's update-check types are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
