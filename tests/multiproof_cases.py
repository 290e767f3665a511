"""The reference of the multi-opening tests (test_ledger_multi_cpu.py, test_gpu_ledger_multi.py, test_gpu_cpp_ledger_multi.py): the
shape of a Merkle multiproof by plain sets, its nodes out of the plain model's tree, its fold by a dict of computed nodes and the verdict
of cstark_account_check_multiproof, all on ledger_model.merge (the oracle's cso_rescue_merge).  It shares nothing with the product."""
import numpy as np

import ledger_model as LM
from ledger_paths_cases import FILL8, FILL64, bump, interesting_indices, leaf  # noqa: F401

P = LM.P
VALID, INDEX, NODE_COUNT, ROOT = 0, 1, 2, 3     # cstark_multi_verdict (include/cstark.h)


def first_bad_index(depth, indices):
    """the first position whose index is >= 2^depth or not above its predecessor, None for a strictly ascending list"""
    for k, i in enumerate(int(i) for i in indices):
        if i >= 1 << depth or (k and i <= int(indices[k - 1])):
            return k
    return None


def proof_positions(depth, indices):
    """[(level, x)] of the proof nodes in canonical order: level depth first, ascending x within a level"""
    assert first_bad_index(depth, indices) is None
    known, out = set(int(i) for i in indices), []
    for l in range(depth, 0, -1):
        out += [(l, x ^ 1) for x in sorted(known) if x ^ 1 not in known]
        known = set(x >> 1 for x in known)
    return out


def shape(depth, indices):
    """(n_nodes, n_merges): n_merges = the sizes of K_l over the levels l < depth"""
    known, n_merges = set(int(i) for i in indices), 0
    for _ in range(depth):
        known = set(x >> 1 for x in known)
        n_merges += len(known)
    return len(proof_positions(depth, indices)), n_merges


def nodes_from_model(m, indices):
    """the multiproof of `indices` out of the model's tree: [n_nodes][7]"""
    return np.array([m._node(l, x) for l, x in proof_positions(m.depth, indices)], np.uint64).reshape(-1, 7)


def leaves_from_model(m, indices):
    return np.array([m._node(m.depth, int(i)) for i in indices], np.uint64).reshape(-1, 7)


def accounts_from_model(m, indices):
    """(values [count][14], present uint8 [count]) as the ledger states them: zeros for an absent account"""
    values = np.array([m.value.get(int(i), np.zeros(14, np.uint64)) for i in indices], np.uint64).reshape(-1, 14)
    return values, np.array([int(i) in m.value for i in indices], np.uint8)


def fold(depth, indices, leaves, nodes):
    """-> (root, number of merges): every node is taken from the dict of computed nodes or, once each and in order, from the proof"""
    nodes = np.asarray(nodes, np.uint64).reshape(-1, 7)
    positions = proof_positions(depth, indices)
    assert len(positions) == len(nodes)
    have = {(depth, int(i)): np.asarray(d, np.uint64) for i, d in zip(indices, np.asarray(leaves, np.uint64).reshape(-1, 7))}
    given = dict(zip(positions, nodes))
    assert not set(have) & set(given)
    n_merges, level = 0, sorted(int(i) for i in indices)
    for l in range(depth, 0, -1):
        get = lambda x: have[(l, x)] if (l, x) in have else given.pop((l, x))
        parents = sorted(set(x >> 1 for x in level))
        for q in parents:
            have[(l - 1, q)] = LM.merge(get(2 * q), get(2 * q + 1))
            n_merges += 1
        level = parents
    assert not given
    return have[(0, 0)], n_merges


def leaves_of(values, present=None):
    values = np.asarray(values, np.uint64).reshape(-1, 14)
    return np.array([leaf(v, True if present is None else bool(present[k])) for k, v in enumerate(values)], np.uint64).reshape(-1, 7)


def expected_verdict(depth, indices, nodes, root, values=None, present=None, leaves=None):
    """-> (verdict, at, folded root or None, n_merges or None): the first that applies of INDEX, NODE_COUNT, ROOT"""
    assert (values is None) != (leaves is None)
    bad = first_bad_index(depth, indices)
    if bad is not None:
        return INDEX, bad, None, None
    n_nodes, n_merges = shape(depth, indices)
    nodes = np.zeros((0, 7), np.uint64) if nodes is None else np.asarray(nodes, np.uint64).reshape(-1, 7)
    if len(nodes) != n_nodes:
        return NODE_COUNT, n_nodes, None, n_merges
    folded, merges = fold(depth, indices, leaves_of(values, present) if leaves is None else leaves, nodes)
    assert merges == n_merges
    return (VALID if np.array_equal(folded, np.asarray(root, np.uint64).reshape(7)) else ROOT), 0, folded, n_merges


def opened(sc):
    """what the multi-opening tests open of a scenario: ledger_paths_cases.interesting_indices, ascending and distinct"""
    return np.array(sorted(set(int(i) for i in interesting_indices(sc))), np.uint64)
