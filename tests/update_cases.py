"""The reference of the update-check tests (test_account_update_cpu.py, test_gpu_account_update.py, test_gpu_cpp_account_update.py): the
verdict of cstark_account_check_update by two plain folds of multiproof_cases.fold, one over the old leaves and one over the new ones,
and pairs of plain models (ledger_model.py) that differ in chosen accounts.  It shares nothing with the product."""
import numpy as np

import ledger_model as LM
import ledger_scenarios as LS
import multiproof_cases as MC

VALID, INDEX, NODE_COUNT, OLD_ROOT, NEW_ROOT = 0, 1, 2, 3, 4     # cstark_update_verdict (include/cstark.h)


def _flags(present, n):
    return np.ones(n, np.uint8) if present is None else np.asarray(present, np.uint8).reshape(n)


def n_changed(old_values, old_present, new_values, new_present):
    """positions whose (value, presence) differ; two absent positions are equal whatever their value words"""
    old, new = np.asarray(old_values, np.uint64).reshape(-1, 14), np.asarray(new_values, np.uint64).reshape(-1, 14)
    was, now = _flags(old_present, len(old)), _flags(new_present, len(new))
    return sum(1 for k in range(len(old)) if bool(was[k]) != bool(now[k]) or (was[k] and not np.array_equal(old[k], new[k])))


def expected_update(depth, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root=None):
    """-> (verdict, at, fold of the new state or None, n_changed or None): the first that applies of INDEX, NODE_COUNT, OLD_ROOT, NEW_ROOT"""
    bad = MC.first_bad_index(depth, indices)
    if bad is not None:
        return INDEX, bad, None, None
    need, _ = MC.shape(depth, indices)
    nodes = np.zeros((0, 7), np.uint64) if nodes is None else np.asarray(nodes, np.uint64).reshape(-1, 7)
    if len(nodes) != need:
        return NODE_COUNT, need, None, None
    changed = n_changed(old_values, old_present, new_values, new_present)
    old_fold, _ = MC.fold(depth, indices, MC.leaves_of(old_values, old_present), nodes)
    if not np.array_equal(old_fold, np.asarray(old_root, np.uint64).reshape(7)):
        return OLD_ROOT, 0, None, changed
    new_fold, _ = MC.fold(depth, indices, MC.leaves_of(new_values, new_present), nodes)
    if new_root is not None and not np.array_equal(new_fold, np.asarray(new_root, np.uint64).reshape(7)):
        return NEW_ROOT, 0, new_fold, changed
    return VALID, 0, new_fold, changed


def model_pair(depth, have, indices, change, create=(), delete=(), seed=1):
    """(old model, new model) of a tree of `depth` that holds the accounts `have`: in the new model the accounts `change` have other
    balances and nonces, the accounts `create` exist only there and the accounts `delete` only in the old one.  All of change, create and
    delete are among `indices`, what the test opens: everything else is the same in both, so one multiproof serves both."""
    assert set(change) | set(create) | set(delete) <= set(int(i) for i in indices)
    assert set(change) <= set(have) and not set(create) & set(have) and set(delete) <= set(have) and not set(change) & set(delete)
    values = dict(zip(have, LS.account_values([(LS.B + k, k) for k in range(len(have))], seed=seed)))
    fresh = dict(zip(list(change) + list(create), LS.account_values([(7 * k + 1, k + 2) for k in range(len(change) + len(create))], seed=seed + 1)))
    old, new = LM.LedgerModel(depth), LM.LedgerModel(depth)
    for i in have:
        old._write(int(i), values[i])
        if i not in delete:
            new._write(int(i), fresh[i] if i in change else values[i])
    for i in create:
        new._write(int(i), fresh[i])
    return old, new


def states(old, new, indices):
    """(old_values, old_present, new_values, new_present, nodes, old_root, new_root) of a model pair for the ascending indices"""
    old_values, old_present = MC.accounts_from_model(old, indices)
    new_values, new_present = MC.accounts_from_model(new, indices)
    nodes = MC.nodes_from_model(old, indices)
    assert np.array_equal(nodes, MC.nodes_from_model(new, indices)), "the models differ outside the opened accounts"
    return old_values, old_present, new_values, new_present, nodes, old.root(), new.root()
