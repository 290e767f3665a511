"""cstark_account_check_update on the CPU.  The reference of the update tests (update_cases.py: two plain folds of
multiproof_cases.fold) is pinned against the plain model: the opening of a scenario's accounts before its batch and the accounts after it
fold to the model's two roots, and after a set_accounts likewise.  tests/cpp/account_update_plan_check.cpp (a stand-alone program, built
with AddressSanitizer and UBSan and run directly) runs csrc/multiproof_plan.h's update plan on a host block with the host `merge`, as the
kernel runs it."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_scenarios as LS
import multiproof_cases as MC
import update_cases as UC

ROOT = LC.ROOT


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_the_reference_folds_to_the_model_roots(sc):
    m, d = LS.model(sc), sc.depth
    indices = MC.opened(sc)
    old_root, nodes = m.root(), MC.nodes_from_model(m, indices)
    old_values, old_present = MC.accounts_from_model(m, indices)
    assert not isinstance(m.apply(*LS.transfers(sc)), tuple)
    new_values, new_present = MC.accounts_from_model(m, indices)
    new_root = m.root()
    assert np.array_equal(new_root, LS.expected(sc).final_root)
    assert np.array_equal(nodes, MC.nodes_from_model(m, indices)), "a batch among opened accounts leaves the proof nodes alone"
    changed = UC.n_changed(old_values, old_present, new_values, new_present)
    touched = set(i for s, r, _ in sc.transfers for i in (s, r))
    assert 0 < changed <= len(touched)
    got = UC.expected_update(d, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root)
    assert got[:2] == (UC.VALID, 0) and np.array_equal(got[2], new_root) and got[3] == changed
    computed = UC.expected_update(d, indices, old_values, old_present, new_values, new_present, nodes, old_root)
    assert computed[0] == UC.VALID and np.array_equal(computed[2], new_root)
    # then a set_accounts: an absent neighbour comes into being, an account gets another value
    absent = [int(i) for k, i in enumerate(indices) if not new_present[k]]
    fresh = LS.account_values([(5, 6), (7, 8)], seed=77)
    written = ([absent[0]] if absent else []) + [int(sc.indices()[0])]
    m.set_accounts(written, fresh[2 - len(written):])
    after_values, after_present = MC.accounts_from_model(m, indices)
    got = UC.expected_update(d, indices, new_values, new_present, after_values, after_present, nodes, new_root, m.root())
    assert got[:2] == (UC.VALID, 0) and got[3] == len(written) and np.array_equal(got[2], m.root())


def test_reference_verdicts_follow_the_order():
    old, new = UC.model_pair(7, [8, 9, 10, 127], [8, 9, 10, 12, 20], [10], [12], [9])
    indices = np.array([8, 9, 10, 12, 20], np.uint64)
    old_values, old_present, new_values, new_present, nodes, old_root, new_root = UC.states(old, new, indices)
    verdict = lambda idx=indices, nd=nodes, a=old_root, b=new_root: UC.expected_update(7, idx, old_values, old_present, new_values, new_present, nd, a, b)
    assert verdict()[:2] == (UC.VALID, 0) and verdict()[3] == 3 and np.array_equal(verdict()[2], new_root)
    bad_old, bad_new = old_root.copy(), new_root.copy()
    bad_old[0], bad_new[0] = MC.bump(bad_old[0]), MC.bump(bad_new[0])
    assert verdict(a=bad_old) == (UC.OLD_ROOT, 0, None, 3) == verdict(a=bad_old, b=bad_new)
    got = verdict(b=bad_new)
    assert got[:2] == (UC.NEW_ROOT, 0) and np.array_equal(got[2], new_root)
    assert verdict(b=None)[0] == UC.VALID and verdict(a=bad_old, b=None)[0] == UC.OLD_ROOT
    assert verdict(nd=nodes[:-1]) == (UC.NODE_COUNT, len(nodes), None, None) == verdict(nd=nodes[:-1], a=bad_old)
    swapped = np.array([8, 10, 9, 12, 20], np.uint64)
    assert verdict(idx=swapped) == (UC.INDEX, 2, None, None) == verdict(idx=swapped, nd=nodes[:-1], a=bad_old)
    # two absent positions are equal whatever their value words; a present one is not
    twisted = new_values.copy()
    twisted[4, 3] = 99
    assert not old_present[4] and UC.n_changed(old_values, old_present, twisted, new_present) == 3
    assert UC.n_changed(old_values, None, twisted, None) == 4


def test_the_update_plan_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "account_update_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "account_update_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [line.split(",")[0] for line in out.stdout.splitlines()] == ["ok: depth %d" % d for d in (1, 3, 7)], out.stdout


def test_the_header_declares_the_update_check():
    hdr = open(os.path.join(ROOT, "include", "cstark.h")).read()
    assert "cstark_account_check_update(" in hdr
    for k, name in enumerate(("VALID", "INDEX", "NODE_COUNT", "OLD_ROOT", "NEW_ROOT")):
        assert "CSTARK_UPDATE_%s = %d" % (name, k) in hdr
