"""Steered batches for the account ledger: the collisions, balance edges, depths and refusals that the oracle's witness generator never
draws (ledger_cases.CASES are all draws of it).  A scenario is a depth, its accounts (index -> canonical balance, canonical nonce; the
twelve key words are reduced elements from a fixed seed) and its transfers (sender, receiver, canonical delta); accounts that no
transfer names are bystanders, whose stored nodes the batch must read as siblings.  Expectations come from ledger_model.LedgerModel."""
import functools
import random

import numpy as np

import ledger_model as LM

P = LM.P
B = 1000
_PING = (10, 1010, 2000, 0, 2000, 1, 1999, 7)   # a ping-pong a -> b -> a ...: deltas equal to the balance, zero, and one below it


def _pingpong(a, b):
    order = ((a, b), (b, a), (a, b), (b, a), (b, a), (a, b), (a, b), (b, a))
    return [(s, r, dl) for (s, r), dl in zip(order, _PING)]


class Scenario:
    def __init__(self, name, depth, accounts, transfers):
        self.name, self.depth, self.accounts, self.transfers = name, depth, dict(accounts), list(transfers)

    @property
    def n_tx(self):
        return len(self.transfers)

    def indices(self):
        return np.array(list(self.accounts), np.uint64)

    def bystanders(self):
        named = set(i for s, r, _ in self.transfers for i in (s, r))
        return [i for i in self.accounts if i not in named]

    @functools.lru_cache(maxsize=None)
    def prefix(self, n):
        return Scenario("%s[:%d]" % (self.name, n), self.depth, self.accounts, self.transfers[:n])

    def proof_form(self):
        """The form MerkleAir proves: its trace holds a power of two of transfers, so the longest such prefix (8 or 4 transfers where
        the scenario has as many, the 2 or 1 it has otherwise)."""
        n = 1
        while 2 * n <= self.n_tx:
            n *= 2
        return self if n == self.n_tx else self.prefix(n)


SCENARIOS = [
    Scenario("pingpong_siblings", 3, {0: (B, 0), 1: (B, 5)}, _pingpong(0, 1)),
    Scenario("pingpong_halves", 3, {0: (B, 0), 7: (B, 5), 3: (B, 0), 4: (B, 0)}, _pingpong(0, 7)),
    Scenario("same_pair_8", 3, {6: (B, 0), 7: (0, 0)}, [(6, 7, 125)] * 8),
    Scenario("chain_full_balance", 3, {i: (B if i == 0 else 0, i) for i in range(8)}, [(i, i + 1, B) for i in range(7)] + [(7, 0, B)]),
    Scenario("zero_deltas", 7, {i: (0, 0) for i in (0, 1, 64, 127)}, [(0, 127, 0), (127, 1, 0), (64, 0, 0), (1, 64, 0)]),
    Scenario("depth31_edges", 31, {i: (B, P - 2) for i in (0, 2**31 - 1, 2**30, 2**30 - 1)},
             [(0, 2**31 - 1, B), (2**30, 2**30 - 1, 1), (2**31 - 1, 2**30, 2 * B), (2**30 - 1, 0, B + 1)]),
    Scenario("receiver_wraps_p", 3, {2: (P - 1, P - 1), 5: (P - 1, 0)}, [(2, 5, P - 1), (5, 2, P - 2)]),
    Scenario("depth1_busy", 1, {0: (B, 0), 1: (B, 0)}, [(0, 1, B), (1, 0, 2 * B), (0, 1, 2 * B)]),
    Scenario("single_deep", 15, {12345: (B, 0), 12344: (1, 1), 0: (B, 0), 2**15 - 1: (B, 0)}, [(12345, 12344, B)]),
    Scenario("bystander_siblings", 7, {i: (B, 0) for i in (10, 11, 20, 21, 8, 9, 22, 23, 127)}, [(10, 21, 1), (11, 20, 2), (21, 10, 3), (20, 11, 4)]),
]
BY_NAME = {sc.name: sc for sc in SCENARIOS}
assert sorted(sc.name for sc in SCENARIOS if sc.bystanders()) == ["bystander_siblings", "pingpong_halves", "single_deep"]


def _late(name, bad):
    """seven transfers among accounts 0, 1 and 2, then one that cannot be applied, between accounts the seven have changed"""
    good = [(0, 1, 600), (1, 2, 100), (2, 0, 50), (0, 1, 450), (1, 0, 1), (1, 2, 949), (2, 1, 7)]    # leaves 0:1, 1:7, 2:1092
    return Scenario(name, 7, {0: (B, 0), 1: (0, 3), 2: (100, 0)}, good + [bad])


# (scenario, index of the refused transfer, reason)
REFUSALS = [
    (Scenario("debit_then_short", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, 600), (0, 1, 600)]), 1, LM.BALANCE),
    (Scenario("credit_swapped", 3, {0: (B, 0), 1: (0, 0), 2: (0, 0)}, [(1, 2, B), (0, 1, B)]), 0, LM.BALANCE),
    (Scenario("one_above_balance_first", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, B + 1), (1, 0, 0)]), 0, LM.BALANCE),
    (Scenario("one_above_balance_last_of_8", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, 100)] * 7 + [(0, 1, B - 700 + 1)]), 7, LM.BALANCE),
    (Scenario("precedence_index_over_self", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, 1), (8, 8, 1)]), 1, LM.INDEX_RANGE),
    (Scenario("precedence_self_over_absent", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, 1), (5, 5, 1)]), 1, LM.SELF_TRANSFER),
    (Scenario("precedence_absent_over_balance", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, 1), (0, 5, 2 * B)]), 1, LM.ABSENT),
    (_late("late_index", (0, 128, 1)), 7, LM.INDEX_RANGE),
    (_late("late_self", (1, 1, 1)), 7, LM.SELF_TRANSFER),
    (_late("late_absent", (3, 1, 0)), 7, LM.ABSENT),
    (_late("late_balance", (0, 2, 2)), 7, LM.BALANCE),
]
# accepted only thanks to an earlier credit, or because delta equals the balance exactly: these must NOT be refused
ACCEPTED = [
    Scenario("credit_then_enough", 3, {0: (B, 0), 1: (0, 0), 2: (0, 0)}, [(0, 1, B), (1, 2, B)]),
    Scenario("exact_balance_last_of_8", 3, {0: (B, 0), 1: (0, 0)}, [(0, 1, 100)] * 7 + [(0, 1, B - 700)]),
]


def account_values(balances_nonces, seed=0x1ED6E2):
    """[count][14] words in memory form: twelve key words from the seed, then each row's canonical (balance, nonce)"""
    rng = random.Random(seed)
    rows = [[rng.randrange(P) for _ in range(12)] + list(bn) for bn in balances_nonces]
    v = LM._oracle().to_mont(np.array(rows, np.uint64)).reshape(-1, 14)
    v.flags.writeable = False
    return v


@functools.lru_cache(maxsize=None)
def values(sc):
    """the accounts' values in the order of sc.indices()"""
    return account_values(sc.accounts.values())


def transfers(sc, lo=0, hi=None):
    """the arrays of the scenario's transfers [lo, hi)"""
    return transfer_arrays(sc.transfers[lo:hi], lo)


def transfer_arrays(tr, lo=0):
    """(s_indices, r_indices, deltas in memory form, sig_rx, sig_s) of a list of (sender, receiver, canonical delta); the signatures
    are arbitrary words (numbered from transfer `lo`) that the ledger must copy through"""
    n = len(tr)
    s, r = np.array([t[0] for t in tr], np.uint64), np.array([t[1] for t in tr], np.uint64)
    deltas = LM._oracle().to_mont(np.array([t[2] for t in tr], np.uint64))
    t = np.arange(lo, lo + n, dtype=np.uint64)
    sig_rx = (t[:, None] * np.uint64(6) + np.arange(6, dtype=np.uint64)[None, :] + np.uint64(1)).astype(np.uint64)
    sig_s = ((t[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64)[None, :]) % np.uint64(251)).astype(np.uint8)
    return s, r, deltas, sig_rx, sig_s


def model(sc):
    """a fresh model that holds the scenario's accounts"""
    m = LM.LedgerModel(sc.depth)
    m.set_accounts(sc.indices(), values(sc))
    return m


class Expected:
    """What the model says of a scenario: the root before the batch, the batch's witness (or its refusal) and the accounts after it.
    Computed once per scenario and shared; nothing in it is written to."""

    def __init__(self, sc):
        m = model(sc)
        self.initial_root = m.root()
        got = m.apply(*transfers(sc))
        self.refusal = got if isinstance(got, tuple) else None
        self.witness = None if self.refusal else got
        self.final_root = m.root()
        self.final_values = m.accounts(sc.indices())
        for a in [self.initial_root, self.final_root, self.final_values] + ([getattr(got, f) for f in got.FIELDS] if self.witness else []):
            a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def expected(sc):
    return Expected(sc)
