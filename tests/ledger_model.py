"""A plain model of the account ledger: the transfer loop of TransactionMetadata::build_random (src/lib.rs:341-422) over a dict-backed
sparse tree, sequential and unoptimised.  It is the reference of the steered ledger tests (ledger_scenarios.py,
test_ledger_steered_cpu.py, test_gpu_ledger_steered.py) and shares nothing with the product: digests come from the oracle's
cso_rescue_merge (pinned by test_oracle_field.py), balances and nonces are Python integers mod p."""
import functools

import numpy as np

P = 2**62 + 2**56 + 2**55 + 1

# cstark_ledger_reason (include/cstark.h); a batch is refused at its first transfer, in transfer order, that matches one of them, and
# with the first reason in this order that the transfer matches
INDEX_RANGE, SELF_TRANSFER, ABSENT, BALANCE = 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def merge(left, right):
    O = _oracle()
    a, b, out = np.array(left, np.uint64), np.array(right, np.uint64), np.zeros(7, np.uint64)
    assert a.shape == b.shape == (7,)
    O.lib().cso_rescue_merge(O._p(a), O._p(b), O._p(out))
    return out


def canonical(word):
    """memory form -> Python integer"""
    return int(_oracle().from_mont(np.array([word], np.uint64))[0])


def memory(value):
    """Python integer -> memory form"""
    return _oracle().to_mont(np.array([value % P], np.uint64))[0]


class LedgerModel:
    def __init__(self, depth):
        self.depth = depth
        self.node = [dict() for _ in range(depth + 1)]     # node[level][index]: level 0 = the root, level depth = the leaves
        self.value = {}                                     # leaf index -> 14 words, memory form
        self.empty = [None] * (depth + 1)                   # the digest of an empty subtree rooted at each level
        self.empty[depth] = np.zeros(7, np.uint64)
        for l in range(depth, 0, -1):
            self.empty[l - 1] = merge(self.empty[l], self.empty[l])

    def _node(self, level, x):
        return self.node[level].get(x, self.empty[level])

    def _write(self, index, value):
        """the account's value, its leaf and the path above it"""
        value = np.array(value, np.uint64).reshape(14)
        self.value[index] = value
        d = self.depth
        self.node[d][index] = merge(value[0:7], value[7:14])
        x = index
        for l in range(d, 0, -1):
            x >>= 1
            self.node[l - 1][x] = merge(self._node(l, 2 * x), self._node(l, 2 * x + 1))

    def _path(self, index):
        """[leaf, sibling at level depth, sibling at level depth - 1, ..., sibling at level 1]"""
        d = self.depth
        return np.array([self._node(d, index)] + [self._node(d - k, (index >> k) ^ 1) for k in range(d)], np.uint64)

    def set_accounts(self, indices, values):
        values = np.asarray(values, np.uint64).reshape(-1, 14)
        assert len(indices) == len(values)
        for i, v in zip(indices, values):
            assert 0 <= int(i) < 1 << self.depth
            self._write(int(i), v)

    def root(self):
        return self._node(0, 0).copy()

    def accounts(self, indices):
        return np.array([self.value[int(i)] for i in indices], np.uint64).reshape(-1, 14)

    def n_nodes(self):
        """nodes the tree holds, all levels"""
        return sum(len(level) for level in self.node)

    def copy(self):
        m = LedgerModel.__new__(LedgerModel)
        m.depth, m.empty = self.depth, self.empty
        m.node = [dict(level) for level in self.node]
        m.value = dict(self.value)
        return m

    def apply(self, s, r, deltas, sig_rx=None, sig_s=None):
        """The batch's witness (an oracle.TxWitness: eleven arrays, final_root among them), or (index, reason) of the first transfer that
        cannot be applied, with the model as it was before the call.  deltas are in memory form."""
        O = _oracle()
        n, d = len(s), self.depth
        w = O.TxWitness(n, d)
        w.s_indices[:] = np.asarray(s, np.uint64)
        w.r_indices[:] = np.asarray(r, np.uint64)
        w.deltas[:] = np.asarray(deltas, np.uint64)
        if sig_rx is not None:
            w.sig_rx[:] = sig_rx
        if sig_s is not None:
            w.sig_s[:] = sig_s
        before = (self.node, self.value)
        self.node, self.value = [dict(level) for level in self.node], dict(self.value)
        for t in range(n):
            si, ri, delta = int(s[t]), int(r[t]), canonical(deltas[t])
            reason = 0
            if si >= 1 << d or ri >= 1 << d:
                reason = INDEX_RANGE
            elif si == ri:
                reason = SELF_TRANSFER
            elif si not in self.value or ri not in self.value:
                reason = ABSENT
            elif delta > canonical(self.value[si][12]):
                reason = BALANCE
            if reason:
                self.node, self.value = before
                return t, reason
            w.initial_roots[t] = self.root()
            w.s_old_values[t], w.r_old_values[t] = self.value[si], self.value[ri]
            w.s_paths[t] = self._path(si)
            sv, rv = self.value[si].copy(), self.value[ri].copy()
            sv[12] = memory(canonical(sv[12]) - delta)
            sv[13] = memory(canonical(sv[13]) + 1)
            rv[12] = memory(canonical(rv[12]) + delta)
            self._write(si, sv)
            self._write(ri, rv)
            w.r_paths[t] = self._path(ri)
        w.final_root[:] = self.root()
        return w
