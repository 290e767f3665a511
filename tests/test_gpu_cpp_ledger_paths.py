"""cstark::Ledger::open and cstark::check_account_paths (include/cstark.hpp): tests/cpp/ledger_paths_mirror.cpp, written against the
header and compiled with g++, opens two accounts and one absent index of case (2 transfers, depth 3, seed 2), checks the opening, changes
one word and checks again.  The opened paths are the plain model's, the verdicts and folded roots the plain fold's."""
import os
import re
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import ledger_paths_cases as PC

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "ledger_paths_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ledger_paths_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_opening_and_check_follow_the_reference(tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = re.match(r"as_stored=1 indices=(\d+),(\d+),(\d+) honest=(\d),(\d),(\d) changed=(\d),(\d),(\d)\n", res.stdout)
    assert got, res.stdout
    numbers = [int(g) for g in got.groups()]
    indices, honest, changed = numbers[:3], numbers[3:6], numbers[6:]
    w = LC.generated((2, 3, 2))
    have, values = LC.initial_accounts(w)
    m = LM.LedgerModel(3)
    m.set_accounts(have, values)
    assert [i in m.value for i in indices] == [True, False, True]
    paths = np.fromfile(prefix + ".paths", np.uint64).reshape(3, 4, 7)
    root = np.fromfile(prefix + ".root", np.uint64)
    assert np.array_equal(root, m.root()) and np.array_equal(root, w.initial_roots[0])
    assert np.array_equal(paths, np.array([m._path(i) for i in indices], np.uint64))
    account = lambda i: (m.value.get(i, np.zeros(14, np.uint64)), i in m.value)
    assert honest == [PC.expected_verdict(i, paths[k], 3, root, *account(i)) for k, i in enumerate(indices)] == [PC.VALID] * 3
    tampered = paths.copy()
    tampered[1, 2, 5] ^= np.uint64(1)
    assert changed == [PC.expected_verdict(i, tampered[k], 3, root, *account(i)) for k, i in enumerate(indices)] == [PC.VALID, PC.ROOT, PC.VALID]
    folded = np.fromfile(prefix + ".folded", np.uint64).reshape(3, 7)
    assert np.array_equal(folded, np.array([PC.fold(i, tampered[k], 3) for k, i in enumerate(indices)], np.uint64))


def test_cpp_ledger_paths_mirror_compiles():
    """CPU check: the header's opening types are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
