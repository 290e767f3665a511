"""The ledger's multi-openings on the CPU.  The reference of the multiproof tests (multiproof_cases.py) is pinned against the plain
model: the multiproof the model gives folds to the model's root before and after a batch, its nodes are the siblings the model's own
paths hold, and its counts are those of a brute-force walk over every node of the opened paths.  tests/cpp/ledger_multi_check.cpp (a
stand-alone program, built with AddressSanitizer and UBSan and run directly) runs csrc/multiproof_plan.h's two plans on a host pool with
the host `merge`."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_scenarios as LS
import multiproof_cases as MC

ROOT = LC.ROOT


def _brute_counts(depth, indices):
    """(n_nodes, n_merges) from the paths one by one: the nodes ON a path are computed, the siblings that are on no path are given"""
    on_path = set((depth - k, int(i) >> k) for i in indices for k in range(depth + 1))
    siblings = set((depth - k, (int(i) >> k) ^ 1) for i in indices for k in range(depth))
    return len(siblings - on_path), sum(1 for l, _ in on_path if l < depth)


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_model_multiproofs_fold_to_the_model_root(sc):
    m, d = LS.model(sc), sc.depth
    indices = MC.opened(sc)
    assert set(sc.accounts) <= set(int(i) for i in indices) and MC.first_bad_index(d, indices) is None
    for when in ("before", "after"):
        root = m.root()
        nodes = MC.nodes_from_model(m, indices)
        values, present = MC.accounts_from_model(m, indices)
        leaves = MC.leaves_of(values, present)
        assert np.array_equal(leaves, MC.leaves_from_model(m, indices)), when
        folded, merges = MC.fold(d, indices, leaves, nodes)
        assert np.array_equal(folded, root), when
        assert (len(nodes), merges) == MC.shape(d, indices) == _brute_counts(d, indices), when
        # every proof node (l, x ^ 1) is entry d - l + 1 of the model's path of an opened index under x
        for (l, y), digest in zip(MC.proof_positions(d, indices), nodes):
            under = [int(i) for i in indices if int(i) >> (d - l) == y ^ 1]
            assert under, (when, l, y)
            for i in under:
                assert np.array_equal(m._path(i)[d - l + 1], digest), (when, l, y, i)
        got = MC.expected_verdict(d, indices, nodes, root, values, present)
        assert got[:2] == (MC.VALID, 0) and np.array_equal(got[2], root) and got[3] == merges
        if when == "before":
            assert not isinstance(m.apply(*LS.transfers(sc)), tuple)
    assert np.array_equal(root, LS.expected(sc).final_root)


def test_shape_edge_cases():
    for d in (1, 3, 7, 15, 31):
        for i in (0, (1 << d) - 1, (1 << d) // 3):
            assert MC.shape(d, [i]) == (d, d)                                   # one leaf: a path
    assert MC.shape(3, list(range(8))) == (0, 7)                                # all leaves: no node, the whole tree rebuilt
    assert MC.proof_positions(3, list(range(8))) == []
    assert MC.shape(3, [4, 5]) == (2, 3) and MC.proof_positions(3, [4, 5]) == [(2, 3), (1, 0)]      # two siblings
    assert MC.shape(3, [0, 7]) == (4, 5)                                        # the two ends share the root only
    assert MC.proof_positions(3, [0, 7]) == [(3, 1), (3, 6), (2, 1), (2, 2)]
    assert MC.shape(31, [0, 2**31 - 1]) == (60, 61)
    assert MC.shape(7, list(range(64, 128))) == (1, 63 + 1)                     # an aligned run: one subtree and its one sibling
    assert MC.proof_positions(7, list(range(64, 128))) == [(1, 0)]
    assert MC.shape(7, list(range(33, 97))) == _brute_counts(7, range(33, 97))  # the same run unaligned
    assert MC.proof_positions(7, list(range(33, 97)))[:2] == [(7, 32), (7, 97)]
    # the figures of the design note: 65,536 consecutive accounts at depth 31 are 15 siblings
    assert MC.shape(31, np.arange(1 << 16, 1 << 17, dtype=np.uint64)) == (15, 65535 + 15)


def test_reference_verdicts_follow_the_order():
    sc = LS.BY_NAME["bystander_siblings"]
    m, d = LS.model(sc), sc.depth
    indices = np.array([10, 12, 20], np.uint64)
    nodes, root = MC.nodes_from_model(m, indices), m.root()
    values, present = MC.accounts_from_model(m, indices)
    n_nodes, n_merges = MC.shape(d, indices)
    verdict = lambda idx=indices, nd=nodes, r=root, **kw: MC.expected_verdict(d, idx, nd, r, **(kw or dict(values=values, present=present)))[:2]
    assert verdict() == (MC.VALID, 0) == verdict(leaves=MC.leaves_from_model(m, indices))
    bad_root = root.copy()
    bad_root[0] = MC.bump(bad_root[0])
    assert verdict(r=bad_root) == (MC.ROOT, 0)
    assert verdict(nd=nodes[:-1]) == (MC.NODE_COUNT, n_nodes) == verdict(nd=nodes[:-1], r=bad_root)
    swapped, repeated, beyond = np.array([12, 10, 20], np.uint64), np.array([10, 12, 12], np.uint64), np.array([10, 12, 128], np.uint64)
    # INDEX before NODE_COUNT before ROOT
    assert verdict(idx=swapped) == (MC.INDEX, 1) == verdict(idx=swapped, nd=nodes[:-1], r=bad_root)
    assert verdict(idx=repeated) == (MC.INDEX, 2) and verdict(idx=beyond, nd=nodes[:2]) == (MC.INDEX, 2)
    assert verdict(values=values, present=np.array([1, 1, 1], np.uint8)) == (MC.ROOT, 0)     # 12 holds no account
    assert MC.expected_verdict(d, indices, nodes, root, values, present)[3] == n_merges
    assert MC.expected_verdict(d, indices, nodes[:-1], root, values, present)[2:] == (None, n_merges)
    assert MC.expected_verdict(d, swapped, nodes, root, values, present)[2:] == (None, None)


def test_the_plans_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_multi_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_multi_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [line.split(",")[0] for line in out.stdout.splitlines()] == ["ok: depth %d" % d for d in (1, 2, 3, 7, 15, 31)], out.stdout


def test_the_header_declares_the_multi_opening_calls():
    hdr = open(os.path.join(ROOT, "include", "cstark.h")).read()
    for name in ("cstark_account_multiproof_shape", "cstark_ledger_open_multi", "cstark_account_check_multiproof"):
        assert name + "(" in hdr
