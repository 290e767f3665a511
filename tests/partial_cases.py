"""Shared by the partial-ledger tests (test_ledger_partial_cpu.py, test_gpu_ledger_partial.py, test_gpu_cpp_ledger_partial.py): what is
opened of a scenario, and the sets a partial ledger must store, by plain sets over multiproof_cases.  It shares nothing with the product."""
import numpy as np

import multiproof_cases as MC


def opened(sc):
    """the scenario's accounts, every in-range index its transfers name (absent ones among them: an opened absent account is refused as
    ABSENT, an unopened one as UNKNOWN) and a few absent neighbours, ascending and distinct"""
    size = 1 << sc.depth
    named = [i for s, r, _ in sc.transfers for i in (s, r) if 0 <= i < size]
    return np.array(sorted(set(int(i) for i in MC.opened(sc)) | set(named)), np.uint64)


def fold_positions(depth, indices):
    """[(level, x)] of the computed nodes of the fold: every proper ancestor of an opened leaf"""
    return sorted(set((depth - k, int(i) >> k) for i in indices for k in range(1, depth + 1)))


def stored_positions(depth, indices, present):
    """what a partial ledger stores: the present opened leaves, the proof nodes, the fold nodes"""
    leaves = [(depth, int(i)) for i, p in zip(indices, present) if p]
    return sorted(set(leaves) | set(MC.proof_positions(depth, indices)) | set(fold_positions(depth, indices)))


def known_by_opaque_ancestor(depth, indices):
    """the leaves without an opaque (proof node) ancestor-or-self, by brute force over the whole tree: small depths only"""
    opaque = set(MC.proof_positions(depth, indices))
    return [x for x in range(1 << depth) if not any((depth - k, x >> k) in opaque for k in range(depth + 1))]
