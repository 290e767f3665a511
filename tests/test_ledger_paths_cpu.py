"""The read side of the account ledger on the CPU.  The reference of the path tests (ledger_paths_cases.fold) is pinned against the
plain model: every path the model gives folds to the model's root, before and after a batch.  tests/cpp/ledger_open_check.cpp (a
stand-alone program, built with AddressSanitizer and UBSan and run directly) runs csrc/ledger_plan.h's plan_open on a host pool and
folds every opened path with the host `merge`."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_paths_cases as PC
import ledger_scenarios as LS

ROOT = LC.ROOT


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_model_paths_fold_to_the_model_root(sc):
    m = LS.model(sc)
    indices = PC.interesting_indices(sc)
    assert set(sc.accounts) <= set(int(i) for i in indices)
    assert len(sc.accounts) == 1 << sc.depth or any(int(i) not in sc.accounts for i in indices)
    for when in ("before", "after"):
        root = m.root()
        for i in indices:
            path = m._path(int(i))
            assert np.array_equal(PC.fold(i, path, sc.depth), root), (when, int(i))
            present = int(i) in m.value
            assert np.array_equal(path[0], PC.leaf(m.value[int(i)] if present else None, present)), (when, int(i))
            assert PC.expected_verdict(i, path, sc.depth, root, m.value.get(int(i), np.zeros(14, np.uint64)), present) == PC.VALID
        if when == "before":
            assert not isinstance(m.apply(*LS.transfers(sc)), tuple)
    assert not np.array_equal(root, LS.expected(sc).initial_root) and np.array_equal(root, LS.expected(sc).final_root)


def test_reference_verdicts_follow_the_order():
    sc = LS.BY_NAME["bystander_siblings"]
    m = LS.model(sc)
    d, i, root = sc.depth, 10, m.root()
    path, value = m._path(i), m.value[i]
    assert PC.expected_verdict(i, path, d, root, value) == PC.VALID == PC.expected_verdict(i, path, d, root)
    bad_leaf = path.copy()
    bad_leaf[0, 0] = PC.bump(bad_leaf[0, 0])
    assert PC.expected_verdict(i, bad_leaf, d, root, value) == PC.LEAF and PC.expected_verdict(i, bad_leaf, d, root) == PC.ROOT
    assert PC.expected_verdict(i, path, d, root, value, present=False) == PC.LEAF
    assert PC.expected_verdict(i ^ 4, path, d, root, value) == PC.ROOT
    assert PC.expected_verdict(i + 128, path, d, root, value) == PC.INDEX_RANGE == PC.expected_verdict(i + 128, bad_leaf, d, root, value)
    assert np.array_equal(PC.fold(i + 128, path, d), root)      # the fold reads bits 0 .. depth - 1 only


def test_plan_open_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_open_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_open_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [line.split(",")[0] for line in out.stdout.splitlines()] == ["ok: depth %d" % d for d in (1, 2, 3, 7, 15, 31)], out.stdout
