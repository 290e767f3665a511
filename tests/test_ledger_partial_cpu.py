"""The partial ledger on the CPU.  tests/cpp/ledger_partial_plan_check.cpp (a stand-alone program, built with AddressSanitizer and UBSan
and run directly) runs csrc/multiproof_plan.h's seed plan and csrc/ledger_plan.h's plans on a partial index with the host `merge`.  The
sets the GPU tests expect of a partial ledger (partial_cases.py) are pinned here by plain sets: what is stored, and that the leaves without
an opaque ancestor are exactly the opened ones."""
import os
import subprocess

import pytest

import ledger_cases as LC
import ledger_scenarios as LS
import multiproof_cases as MC
import partial_cases as PC

ROOT = LC.ROOT

SETS = [(d, name, idx) for d in (1, 3, 7) for name, idx in (
    ("one_leaf", [(1 << d) // 3]), ("sibling_pair", [(1 << d) - 2, (1 << d) - 1]), ("all_leaves", list(range(1 << d))),
    ("alternating", list(range(0, 1 << d, 2))))]


@pytest.mark.parametrize("depth,name,indices", SETS, ids=lambda v: v if isinstance(v, str) else None)
def test_known_is_opened_and_stored_is_leaves_proof_and_fold(depth, name, indices):
    assert PC.known_by_opaque_ancestor(depth, indices) == sorted(indices)
    proof, fold = MC.proof_positions(depth, indices), PC.fold_positions(depth, indices)
    assert len(proof) == MC.shape(depth, indices)[0] and len(fold) == MC.shape(depth, indices)[1]
    assert not set(proof) & set(fold), "a proof node is never computed"
    # no opened leaf's path holds a proof node: no write ever reaches one
    on_path = set((depth - k, i >> k) for i in indices for k in range(depth + 1))
    assert not on_path & set(proof)
    # every sibling a path reads is stored or is an opened (absent: empty) leaf
    present = [i % 3 != 1 for i in indices]
    stored = set(PC.stored_positions(depth, indices, present))
    for i in indices:
        for k in range(depth):
            sibling = (depth - k, (i >> k) ^ 1)
            assert sibling in stored or (k == 0 and (i ^ 1) in indices), (i, k)
    assert len(stored) == sum(present) + len(proof) + len(fold)
    if name == "all_leaves":
        assert not proof


@pytest.mark.parametrize("sc", LS.SCENARIOS + [sc for sc, _, _ in LS.REFUSALS], ids=lambda sc: sc.name)
def test_what_the_gpu_tests_open(sc):
    opened = PC.opened(sc)
    assert MC.first_bad_index(sc.depth, opened) is None
    named = set(i for s, r, _ in sc.transfers for i in (s, r) if i < 1 << sc.depth)
    assert set(sc.accounts) | named <= set(int(i) for i in opened)


def test_the_plans_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_partial_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_partial_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [line.split(",")[0] for line in out.stdout.splitlines()] == ["ok: depth %d" % d for d in (1, 3, 7)], out.stdout


def test_the_header_declares_the_partial_ledger_calls():
    hdr = open(os.path.join(ROOT, "include", "cstark.h")).read()
    for name in ("cstark_ledger_create_partial", "cstark_ledger_known", "cstark_ledger_partial_info"):
        assert name + "(" in hdr
    assert "CSTARK_LEDGER_UNKNOWN = 6" in hdr
