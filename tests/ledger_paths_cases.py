"""The reference of the account-path tests (test_ledger_paths_cpu.py, test_gpu_ledger_paths.py, test_gpu_cpp_ledger_paths.py): a plain
fold of an authentication path, the leaf rule and the verdict of cstark_account_check_paths, all on ledger_model.merge (the oracle's
cso_rescue_merge).  It shares nothing with the product."""
import numpy as np

import ledger_model as LM

P = LM.P
VALID, INDEX_RANGE, LEAF, ROOT = 0, 1, 2, 3     # cstark_path_verdict (include/cstark.h)
FILL8, FILL64 = 0xA5, 0xA5A5A5A5A5A5A5A5       # what every output buffer holds before a call


def fold(index, path, depth):
    """[leaf, sibling at level depth, ..., sibling at level 1] -> the root, by bits 0 .. depth - 1 of the index (LedgerModel._write)"""
    path = np.asarray(path, np.uint64).reshape(depth + 1, 7)
    cur = path[0].copy()
    for k in range(depth):
        cur = LM.merge(path[k + 1], cur) if (int(index) >> k) & 1 else LM.merge(cur, path[k + 1])
    return cur


def leaf(value, present=True):
    """the leaf digest of an account: merge of the two halves of its value, all-zero for an absent account"""
    if not present:
        return np.zeros(7, np.uint64)
    value = np.asarray(value, np.uint64).reshape(14)
    return LM.merge(value[0:7], value[7:14])


def expected_verdict(index, path, depth, root, value=None, present=True):
    """the first that applies of INDEX_RANGE, LEAF (only with a value: digest mode has no leaf test), ROOT"""
    path = np.asarray(path, np.uint64).reshape(depth + 1, 7)
    if int(index) >> depth:
        return INDEX_RANGE
    if value is not None and not np.array_equal(path[0], leaf(value, present)):
        return LEAF
    if not np.array_equal(fold(index, path, depth), np.asarray(root, np.uint64).reshape(7)):
        return ROOT
    return VALID


def bump(word):
    """(word + 1) mod p: another reduced word"""
    return np.uint64((int(word) + 1) % P)


def interesting_indices(sc):
    """what the tests open of a scenario: its accounts (bystanders among them), their absent neighbours, the two ends of the tree and
    one index twice"""
    size = 1 << sc.depth
    have = [int(i) for i in sc.accounts]
    near = [j for i in have for j in (i ^ 1, i + 2, i - 2) if 0 <= j < size and j not in sc.accounts]
    out = have + sorted(set(near))[:6] + [0, size - 1, have[0]]
    return np.array(out, np.uint64)
