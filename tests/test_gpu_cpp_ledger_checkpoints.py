"""The checkpoints and the audit of cstark::Ledger (include/cstark.hpp): tests/cpp/ledger_checkpoint_mirror.cpp, written against the
header and compiled with g++, takes a checkpoint, applies case (2 transfers, depth 3, seed 2), opens all accounts under the checkpoint's
root and under the new one, audits both states, reverts, applies again and releases.  Paths and roots are the plain model's."""
import os
import re
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM

ROOT = LC.ROOT
PKG = os.path.join(ROOT, "certificate-stark_amd")


def build_program(tmp):
    exe = os.path.join(tmp, "ledger_checkpoint_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ledger_checkpoint_mirror.cpp"), "-o", exe, "-pthread", "-L", PKG, "-lcstark_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_cpp_checkpoint_open_at_revert_and_audit_follow_the_model(tmp_path):
    exe = build_program(str(tmp_path))
    prefix = str(tmp_path / "out")
    res = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = re.match(r"accounts=(\d+) checkpoint=1 applied=1 opened=1 valid=1 audited=1 reverted=1 reapplied=1 gone=1 nodes=(\d+) held=0 free=(\d+)\n", res.stdout)
    assert got, res.stdout
    # every account is named by a transfer, so the second apply moved every node to a fresh slot: the release frees one old slot per node
    assert got.group(3) == got.group(2)
    w = LC.generated((2, 3, 2))
    have, values = LC.initial_accounts(w)
    m = LM.LedgerModel(3)
    m.set_accounts(have, values)
    before = m.copy()
    assert not isinstance(m.apply(w.s_indices, w.r_indices, w.deltas), tuple)
    order = sorted(int(i) for i in have)
    assert int(got.group(1)) == len(order) and int(got.group(2)) == m.n_nodes()
    n = len(order)
    old_paths = np.fromfile(prefix + ".old_paths", np.uint64).reshape(n, 4, 7)
    new_paths = np.fromfile(prefix + ".new_paths", np.uint64).reshape(n, 4, 7)
    roots = np.fromfile(prefix + ".roots", np.uint64).reshape(4, 7)
    assert np.array_equal(old_paths, np.array([before._path(i) for i in order], np.uint64))
    assert np.array_equal(new_paths, np.array([m._path(i) for i in order], np.uint64))
    assert np.array_equal(roots, np.array([before.root(), m.root(), before.root(), m.root()], np.uint64))
    assert not np.array_equal(before.root(), m.root())


def test_cpp_ledger_checkpoint_mirror_compiles():
    """CPU check: the header's checkpoint and audit members are self-contained C++17 and link against the library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert os.path.exists(build_program(tmp))
