"""Cases of the account-ledger tests (test_ledger_cpu.py, test_gpu_ledger.py, test_gpu_cpp_ledger.py): the oracle's generated witnesses,
the accounts a ledger must hold before the batch, and the accounts it must hold after it."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n_tx, depth, seed): 1 and 3 transfers give partial waves; 32 transfers on an 8-leaf tree give collisions at every level and sibling
# leaves updated in one batch; depth 1 has the root directly above the leaves; depth 31 is sparse with large indices; 16 and 64
# transfers at depth 15 use the production depth
CASES = [(1, 3, 1), (2, 3, 2), (3, 3, 7), (16, 3, 3), (32, 3, 9), (6, 1, 11), (5, 7, 8), (8, 7, 4), (16, 15, 5), (64, 15, 10), (4, 31, 6)]


def case_id(c):
    return "n%d_d%d_s%d" % c


@functools.lru_cache(maxsize=None)
def generated(case):
    """the oracle's witness of a case; computed once and shared, never written to"""
    from oracle import oracle as O
    O.build()
    w = O.TxWitness.generate(*case)
    for f in w.FIELDS:
        getattr(w, f).flags.writeable = False
    return w


@functools.lru_cache(maxsize=None)
def golden_1024():
    from oracle import oracle as O
    w = O.TxWitness.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))
    for f in w.FIELDS:
        getattr(w, f).flags.writeable = False
    return w


def initial_accounts(w):
    """(indices, values[count][14]): an account's value at its first appearance in s_old_values / r_old_values is its initial value"""
    seen = {}
    for t in range(w.n_tx):
        for idx, val in ((int(w.s_indices[t]), w.s_old_values[t]), (int(w.r_indices[t]), w.r_old_values[t])):
            if idx not in seen:
                seen[idx] = val
    indices = np.array(list(seen.keys()), np.uint64)
    return indices, np.array([seen[int(i)] for i in indices], np.uint64).reshape(-1, 14)


def final_accounts(w, indices):
    """values[count][14] after the batch: the value each account's last transfer left (src/lib.rs:373-375: field arithmetic)"""
    from oracle import oracle as O
    one = O.to_mont(np.array([1], np.uint64))[0]
    s_new, r_new = w.s_old_values.copy(), w.r_old_values.copy()
    s_new[:, 12] = O.fp_sub(w.s_old_values[:, 12].copy(), w.deltas)
    s_new[:, 13] = O.fp_add(w.s_old_values[:, 13].copy(), np.full(w.n_tx, one, np.uint64))
    r_new[:, 12] = O.fp_add(w.r_old_values[:, 12].copy(), w.deltas)
    last = {}
    for t in range(w.n_tx):
        last[int(w.s_indices[t])] = s_new[t]
        last[int(w.r_indices[t])] = r_new[t]
    return np.array([last[int(i)] for i in indices], np.uint64).reshape(-1, 14)


def absent_index(w, indices):
    """a leaf index below 2^depth without an account, or None when every leaf has one"""
    have = set(int(i) for i in indices)
    for i in range(min(1 << w.depth, len(have) + 1)):
        if i not in have:
            return i
    return None


def write_case(path, w, accounts=None, refusal=None):
    """The case as flat little-endian 64-bit words, as tests/cpp/ledger_plan_check.cpp reads it.
    accounts: (indices, values, final_values) where the accounts are not those the witness names (bystanders that no transfer touches).
    refusal: (refused_at, reason) that the plan must answer to the whole batch; w then holds the arrays of transfers [0, refused_at),
    the root they leave in initial_roots[refused_at], and final_values the accounts they leave."""
    if accounts is None:
        indices, values = initial_accounts(w)
        final = final_accounts(w, indices)
    else:
        indices, values, final = (np.asarray(a, np.uint64) for a in accounts)
    absent = absent_index(w, indices)
    head = np.array([w.depth, len(indices), w.n_tx, 2**64 - 1 if absent is None else absent], np.uint64)
    parts = [head, indices, values, final, w.initial_roots, w.final_root, w.s_old_values, w.r_old_values, w.s_indices,
             w.r_indices, w.s_paths, w.r_paths, w.deltas]
    if refusal is not None:
        parts.append(np.array(refusal, np.uint64))
    with open(path, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a, "<u8").tobytes())
