"""Shared by test_gpu_ledger_checkpoints.py and test_gpu_ledger_audit.py: a ledger on the GPU driven side by side with the plain model
(ledger_model.LedgerModel, imported and not edited), whose copy() is taken at the moment of every checkpoint, and the audit's job order
restated from the model alone."""
import ctypes as C
import random

import numpy as np

import ledger_model as LM
import ledger_scenarios as LS

B = 1000
EMPTY, LEAF, INNER = 0, 1, 2     # cstark_ledger_node_kind
DEBUG_EMPTY = 0xFFFFFFFF         # CSTARK_DEBUG_LEDGER_EMPTY

# depth -> (accounts set before the first checkpoint, accounts created under a live checkpoint): 4 to 12 accounts, both ends of the
# tree, siblings, and at depth 31 indices above 2^24
ACCOUNTS = {
    1: ([0, 1], []),
    3: ([0, 1, 5, 7, 4, 6], [2, 3]),
    15: ([0, 1, 5, 2**15 - 1, 2**14, 12345], [2, 2**15 - 2]),
    31: ([0, 2**31 - 1, 2**30, 0x01000003, 5, 0x7F000000], [0x02000002, 0x7F000001]),
}
assert all(4 <= len(a) + len(b) <= 12 or d == 1 for d, (a, b) in ACCOUNTS.items())


def report_tuple(r):
    return (r.consistent, r.n_bad, r.first_kind, r.first_level, r.first_index, r.n_nodes, r.slots_live, r.slots_held, r.slots_free)


class Pair:
    """a Ledger and the model, driven together; `live` holds (checkpoint id, the model's copy at that moment), oldest first"""

    def __init__(self, backend, depth, seed=1):
        from certificate_stark_amd.prover import Ledger
        self.backend, self.depth = backend, depth
        self.led, self.m = Ledger(depth, backend), LM.LedgerModel(depth)
        self.live = []
        self.rng = random.Random(seed * 1000 + depth)
        self.salt = 0
        first, later = ACCOUNTS[depth]
        size = 1 << depth
        ask = list(first) + list(later)
        ask += [i ^ 1 for i in ask] + [first[0], (size // 3) | 1]         # siblings (absent or not), a repeated index, a lone absent leaf
        self.ask = np.array([i for i in ask if i < size], np.uint64)

    def close(self):
        self.led.close()

    def set_accounts(self, indices):
        """new values for these accounts (created or overwritten): balance B, a nonce that differs from call to call"""
        self.salt += 1
        values = LS.account_values([(B, self.salt)] * len(indices), seed=self.salt * 7919 + self.depth)
        self.led.set_accounts(np.array(indices, np.uint64), values)
        self.m.set_accounts(indices, values)

    def batch(self, n, among):
        """n transfers among these accounts: deltas of 0 .. 5 against balances of about B"""
        tr = []
        for _ in range(n):
            s, r = self.rng.sample(list(among), 2)
            tr.append((s, r, self.rng.randrange(6)))
        return LS.transfer_arrays(tr)

    def apply(self, n, among):
        """-> (what the ledger returned, what the model returned)"""
        tr = self.batch(n, among)
        return self.led.apply(tr), self.m.apply(*tr)

    def checkpoint(self):
        cp = self.led.checkpoint()
        self.live.append((cp, self.m.copy()))
        return cp

    def revert(self, cp):
        self.led.revert(cp)
        at = [c for c, _ in self.live].index(cp)
        del self.live[at + 1:]
        self.m = self.live[at][1].copy()

    def release(self, cp):
        self.led.release(cp)
        self.live = [(c, m) for c, m in self.live if c != cp]

    def states(self):
        """(at, model) of every state the ledger can show: the live checkpoints, then the current one"""
        return list(self.live) + [(None, self.m)]

    def assert_all(self):
        """every live checkpoint and the current state: opening, root and audit are the model's; every opened path verifies"""
        for at, m in self.states():
            assert_state(self.led, m, self.ask, at)
        r = self.led.audit()
        assert r.slots_live == self.m.n_nodes()
        if not self.live:
            assert r.slots_held == 0
        return r


def assert_opening(o, m, indices):
    for k, i in enumerate(int(i) for i in indices):
        assert bool(o.present[k]) == (i in m.value), i
        assert np.array_equal(o.values[k], m.value.get(i, np.zeros(14, np.uint64))), i
        assert np.array_equal(o.paths[k], m._path(i)), i
    assert np.array_equal(o.root, m.root())


def assert_state(led, m, indices, at=None):
    o = led.open(indices, at=at)
    assert_opening(o, m, indices)
    assert np.array_equal(led.root(at=at), m.root())
    assert not o.check().any(), "a path opened at a checkpoint does not verify against the checkpoint's root"
    r = led.audit(at=at)
    assert (r.consistent, r.n_bad, r.n_nodes) == (1, 0, m.n_nodes()), report_tuple(r)


# ---- the audit's job order, from the model alone ------------------------------------------------------------------------------------------
def symbol(m, level, x):
    """what the lookup finds for (level, x): the stored node, or the level's empty-subtree digest"""
    return ("node", level, x) if x in m.node[level] else ("empty", level, 0)


def audit_jobs(m):
    """[(kind, level, x, the digests the test reads)] in the order of cstark_ledger_audit: the all-zero test of the empty leaf digest, the
    empty-subtree digests from level depth - 1 down to 0, the leaves by ascending index, the inner nodes from level depth - 1 down to 0
    and by ascending x"""
    d = m.depth
    jobs = [(EMPTY, d, 0, {("empty", d, 0)})]
    jobs += [(EMPTY, l, 0, {("empty", l, 0), ("empty", l + 1, 0)}) for l in range(d - 1, -1, -1)]
    jobs += [(LEAF, d, x, {("node", d, x)}) for x in sorted(m.node[d])]
    for l in range(d - 1, -1, -1):
        jobs += [(INNER, l, x, {("node", l, x), symbol(m, l + 1, 2 * x), symbol(m, l + 1, 2 * x + 1)}) for x in sorted(m.node[l])]
    return jobs


def expected_failures(m, corrupted):
    """-> (n_bad, (kind, level, x) of the first failing job) when the digest `corrupted` (a symbol) is wrong"""
    bad = [(k, l, x) for k, l, x, reads in audit_jobs(m) if corrupted in reads]
    return len(bad), bad[0]


def xor_word(led, symbol_, word, at=0, mask=1):
    """cstark_debug_ledger_xor_word on the digest a symbol names"""
    from certificate_stark_amd import _lib
    kind, level, x = symbol_
    if kind == "empty":
        level, x = DEBUG_EMPTY, level
    return _lib.load_debug().cstark_debug_ledger_xor_word(led._led, C.c_uint64(at), C.c_uint32(level), C.c_uint64(x), C.c_uint32(word), C.c_uint64(mask))
