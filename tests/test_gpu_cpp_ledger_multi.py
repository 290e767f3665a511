"""cstark::Ledger::open_multi and cstark::check_account_multiproof (include/cstark.hpp): tests/cpp/ledger_multi_mirror.cpp, written
against the header and compiled with g++, opens two accounts and one absent index of case (2 transfers, depth 3, seed 2) with one
multiproof, checks it, changes one word and checks again, drops a node and checks again.  The opened nodes are the plain model's, the
verdicts and the folded root the plain fold's."""
import os
import re
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import multiproof_cases as MC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "ledger_multi_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ledger_multi_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_multi_opening_and_check_follow_the_reference(tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = re.match(r"as_stored=1 indices=(\d+),(\d+),(\d+) n_nodes=(\d+) honest=(\d+),(\d+),(\d+),(\d) changed=(\d+),(\d+),(\d+) dropped=(\d+),(\d+)\n",
                   res.stdout)
    assert got, res.stdout
    numbers = [int(g) for g in got.groups()]
    indices, n_nodes, honest, changed, dropped = numbers[:3], numbers[3], numbers[4:8], numbers[8:11], numbers[11:]
    w = LC.generated((2, 3, 2))
    have, values = LC.initial_accounts(w)
    m = LM.LedgerModel(3)
    m.set_accounts(have, values)
    assert indices == sorted(indices) and sorted(i in m.value for i in indices) == [False, True, True]
    nodes = np.fromfile(prefix + ".nodes", np.uint64).reshape(-1, 7)
    root = np.fromfile(prefix + ".root", np.uint64)
    assert np.array_equal(root, m.root()) and np.array_equal(root, w.initial_roots[0])
    assert len(nodes) == n_nodes == MC.shape(3, indices)[0] and np.array_equal(nodes, MC.nodes_from_model(m, indices))
    account_values, present = MC.accounts_from_model(m, indices)
    ref = MC.expected_verdict(3, indices, nodes, root, account_values, present)
    assert honest == [MC.VALID, 0, ref[3], 1] and ref[0] == MC.VALID
    tampered = nodes.copy()
    tampered[-1, 4] ^= np.uint64(1)
    ref = MC.expected_verdict(3, indices, tampered, root, account_values, present)
    assert changed == [MC.ROOT, 0, ref[3]] and ref[0] == MC.ROOT
    assert np.array_equal(np.fromfile(prefix + ".folded", np.uint64), ref[2])
    assert dropped == list(MC.expected_verdict(3, indices, tampered[:-1], root, account_values, present)[:2]) == [MC.NODE_COUNT, n_nodes]


def test_cpp_ledger_multi_mirror_compiles():
    """CPU check: the header's multi-opening types are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
