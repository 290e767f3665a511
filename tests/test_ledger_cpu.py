"""csrc/ledger_plan.h on the CPU: tests/cpp/ledger_plan_check.cpp (a stand-alone program, built with AddressSanitizer and UBSan and
run directly) executes the ledger's job lists with the host `merge` and compares every witness array with the oracle's generator --
the same cases as the GPU test, plus the refusals of the plan, two-call and overwriting set_accounts, and batches that compose."""
import os
import subprocess

import pytest

import ledger_cases as LC

ROOT = LC.ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ledger_plan") / "ledger_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_plan_check.cpp")])
    return exe


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_plan_reproduces_the_generator(checker, case, tmp_path):
    path = str(tmp_path / "case.bin")
    LC.write_case(path, LC.generated(case))
    out = subprocess.run([checker, path], capture_output=True, text=True)
    n_tx, depth, _ = case
    assert out.returncode == 0 and out.stdout.startswith("ok: depth %d," % depth), out.stdout + out.stderr
    assert "%d transfers, %d merges in %d launches" % (n_tx, 2 * n_tx * (depth + 1), depth + 1) in out.stdout


def test_checker_notices_a_wrong_witness(checker, tmp_path):
    """the comparison is live: one flipped word of a sibling digest fails the check"""
    import numpy as np
    w = LC.generated((2, 3, 2)).copy()
    w.r_paths[1, 2, 3] ^= np.uint64(1)
    path = str(tmp_path / "case.bin")
    LC.write_case(path, w)
    out = subprocess.run([checker, path], capture_output=True, text=True)
    assert out.returncode == 1 and "r_paths differ" in out.stdout, out.stdout + out.stderr
