"""The pools of the Ledger.select tests (test_ledger_select_cpu.py, test_gpu_ledger_select.py, test_gpu_cpp_ledger_select.py), in account
numbers, 12 to 25 candidates each: seven accounts k = 0..6 with secret key k + 1, balance 1000 and nonce k, at the leaves INDICES[depth]; leaf ABSENT[depth] has
no account.  A pool is an appliable SKELETON, which is signed as one batch (every candidate for the nonce its sender has when all
before it are accepted), with candidates spliced in or corrupted afterwards: the spliced-in candidates do not shift the nonces the
others signed, as in a real pool.  The reference of every pool is tests/select_model.py."""
import numpy as np

import ledger_model as LM

P = LM.P
N_ACC = 7
INDICES = {3: [0, 1, 6, 7, 3, 4, 2], 7: [0, 100, 127, 99, 64, 33, 2]}
ABSENT = {3: 5, 7: 5}
DEPTHS = (3, 7)
# (sender, receiver, delta) in account numbers.  Senders 0..3 send more than once (k_t > 0), account 0 receives after it has sent.
SKELETON = [(0, 1, 10), (1, 2, 20), (2, 3, 30), (0, 2, 5), (3, 4, 40), (4, 5, 50), (5, 6, 60), (1, 0, 7), (6, 0, 70), (2, 1, 3), (0, 3, 1), (3, 0, 2)]
MORE = [(4, 0, 11), (5, 1, 12), (6, 2, 13), (0, 4, 14), (1, 5, 15), (2, 6, 16), (3, 1, 17), (4, 2, 18), (5, 3, 19), (6, 4, 21), (0, 5, 22), (1, 6, 23)]
# account 1 spends what account 0's transfer brings it; the six transfers after that name neither of them as a sender
CASCADE = [(0, 1, 500), (1, 2, 1400), (2, 3, 30), (1, 4, 5), (3, 4, 1), (0, 5, 1), (4, 5, 50), (5, 6, 60), (6, 4, 70), (2, 6, 3), (3, 2, 2), (4, 6, 1)]


class Entry:
    """one candidate: leaf indices, delta (an integer), the skeleton position whose signature it carries (None: an all-zero one) and
    what is done to that signature: ok, s_bit, rx_plus1, s_bit255, rx_ge_p"""

    def __init__(self, s, r, delta, src=None, sig="ok"):
        self.s, self.r, self.delta, self.src, self.sig = int(s), int(r), int(delta), src, sig


class Pool:
    def __init__(self, depth, skeleton, want=None, pow2=False, partial=False, off_curve=None):
        self.depth, self.skeleton, self.pow2, self.partial, self.off_curve = depth, list(skeleton), pow2, partial, off_curve
        leaf = INDICES[depth]
        self.entries = [Entry(leaf[a], leaf[b], d, src=i) for i, (a, b, d) in enumerate(skeleton)]
        self._want = want

    @property
    def n(self):
        return len(self.entries)

    @property
    def want(self):
        return self.n if self._want is None else self._want

    def leaf(self, k):
        return INDICES[self.depth][k]

    def splice(self, at, s, r, delta, src=None, sig="ok"):
        self.entries.insert(at, Entry(s, r, delta, src, sig))
        return self

    def corrupt(self, at, sig):
        self.entries[at].sig = sig
        return self

    # ---- arrays
    def indices(self):
        return np.array(INDICES[self.depth], np.uint64)

    def values(self, keys):
        """the accounts [7][14] with the given public keys [7][12]"""
        v = np.zeros((N_ACC, 14), np.uint64)
        v[:, :12] = keys
        v[:, 12] = [LM.memory(1000)] * N_ACC
        v[:, 13] = [LM.memory(k) for k in range(N_ACC)]
        return v

    def skeleton_batch(self):
        """(s, r, deltas, secrets) of the skeleton, what Ledger.sign takes"""
        leaf = INDICES[self.depth]
        return (np.array([leaf[a] for a, _, _ in self.skeleton], np.uint64), np.array([leaf[b] for _, b, _ in self.skeleton], np.uint64),
                np.array([LM.memory(d) for _, _, d in self.skeleton], np.uint64), np.array([a + 1 for a, _, _ in self.skeleton], np.uint64))

    def batch(self):
        """(s, r, deltas) of the pool"""
        return (np.array([e.s for e in self.entries], np.uint64), np.array([e.r for e in self.entries], np.uint64),
                np.array([LM.memory(e.delta) for e in self.entries], np.uint64))

    def signatures(self, skel_rx, skel_s):
        """(sig_rx [n][6], sig_s [n][32]) of the pool from the skeleton's signatures"""
        rx, ss = np.zeros((self.n, 6), np.uint64), np.zeros((self.n, 32), np.uint8)
        for t, e in enumerate(self.entries):
            if e.src is not None:
                rx[t], ss[t] = skel_rx[e.src], skel_s[e.src]
            if e.sig == "s_bit":
                ss[t, 9] ^= 0x10
            elif e.sig == "s_bit255":
                ss[t, 31] |= 0x80
            elif e.sig == "rx_plus1":
                rx[t, 0] = np.uint64((int(rx[t, 0]) + 1) % P)
            elif e.sig == "rx_ge_p":
                rx[t, 2] = np.uint64(P + 5)
            elif e.sig != "ok":
                raise ValueError(e.sig)
        return rx, ss

    def known(self):
        """the leaves a partial ledger knows: those the skeleton names"""
        leaf = INDICES[self.depth]
        return sorted({leaf[a] for a, _, _ in self.skeleton} | {leaf[b] for _, b, _ in self.skeleton})


def _skeleton11(depth):
    return Pool(depth, SKELETON[:11], want=16, pow2=True)


def _cascade(depth):
    p = Pool(depth, CASCADE)
    return p.splice(0, p.leaf(0), p.leaf(0), 1)


def _replay(depth):
    p = Pool(depth, SKELETON)
    e = p.entries[1]
    return p.splice(2, e.s, e.r, e.delta, src=1)


def _chunks(depth):
    p = Pool(depth, SKELETON + MORE)
    return p.corrupt(5, "s_bit").corrupt(15, "rx_ge_p").corrupt(18, "rx_plus1")


# name -> builder(depth).  The static refusals are spliced in at position 4 with sender 0, who has sent twice by then, sends again at
# skeleton position 10 and receives at 7, 8 and 11.
CASES = {
    "all_valid": lambda d: Pool(d, SKELETON),
    "want_5": lambda d: Pool(d, SKELETON, want=5),
    "sender_out_of_range": lambda d: Pool(d, SKELETON).splice(4, (1 << d) + 1, INDICES[d][1], 1),
    "receiver_out_of_range": lambda d: Pool(d, SKELETON).splice(4, INDICES[d][0], 1 << d, 1),
    "self_transfer": lambda d: Pool(d, SKELETON).splice(4, INDICES[d][0], INDICES[d][0], 1),
    "absent_sender": lambda d: Pool(d, SKELETON).splice(4, ABSENT[d], INDICES[d][1], 1).splice(9, ABSENT[d], INDICES[d][2], 1),
    "absent_receiver": lambda d: Pool(d, SKELETON).splice(4, INDICES[d][0], ABSENT[d], 1),
    "unknown": lambda d: Pool(d, SKELETON[:6] + SKELETON[9:], partial=True).splice(4, INDICES[d][0], INDICES[d][6], 1),
    "overdraft": lambda d: Pool(d, SKELETON).splice(4, INDICES[d][2], INDICES[d][3], 5000),
    "cascade": _cascade,
    "flipped_s": lambda d: Pool(d, SKELETON).corrupt(3, "s_bit"),
    "rx_plus_one": lambda d: Pool(d, SKELETON).corrupt(3, "rx_plus1"),
    "s_bit_255": lambda d: Pool(d, SKELETON).corrupt(3, "s_bit255"),
    "rx_not_reduced": lambda d: Pool(d, SKELETON).corrupt(3, "rx_ge_p"),
    "replay": _replay,
    "off_curve_key": lambda d: Pool(d, SKELETON, off_curve=2),
    "pow2_11_of_16": _skeleton11,
    "pow2_want_1": lambda d: Pool(d, SKELETON, want=1, pow2=True),
    "chunks_24": _chunks,
}
# what each case is there to show: status -> candidate numbers that must carry it (the model decides everything else)
LANDMARKS = {
    "all_valid": {0: list(range(12))},
    "want_5": {0: [0, 1, 2, 3, 4], 9: list(range(5, 12))},
    "sender_out_of_range": {1: [4], 8: []},
    "receiver_out_of_range": {1: [4], 8: [11], 0: [8, 9, 12]},
    "self_transfer": {2: [4], 8: [11], 0: [8, 9, 12]},
    "absent_sender": {3: [4, 9], 8: []},
    "absent_receiver": {3: [4], 8: [11], 0: [8, 9, 12]},
    "unknown": {6: [4], 8: [8], 0: [9]},
    "overdraft": {4: [4], 8: [10]},
    "cascade": {2: [0], 8: [1, 4, 6], 4: [2], 0: [3, 5, 7, 8, 9, 10, 11, 12]},
    "flipped_s": {5: [3], 8: [10], 0: [7, 8, 11]},
    "rx_plus_one": {5: [3], 8: [10]},
    "s_bit_255": {5: [3], 8: [10]},
    "rx_not_reduced": {5: [3], 8: [10]},
    "replay": {5: [2], 8: [8], 0: [0, 1]},
    # account 2's key changes under signatures made before: its own first candidate (2) has a key off the curve, and the candidates
    # that pay it (1, 3) signed another receiver's key
    "off_curve_key": {5: [1, 2, 3], 8: [7, 9, 10]},
    "pow2_11_of_16": {0: list(range(8)), 9: [8, 9, 10]},
    "pow2_want_1": {0: [0], 9: list(range(1, 12))},
    "chunks_24": {5: [5, 15, 18]},
}


def check_landmarks(name, status):
    """the refusals of a case sit exactly where LANDMARKS says, and the candidates it names as selected are selected"""
    for st, where in LANDMARKS[name].items():
        carriers = [t for t, v in enumerate(status) if v == st]
        assert (set(where) <= set(carriers)) if st == 0 else (carriers == where), (name, st, carriers)


def nothing_selectable(depth):
    """every sender's first candidate carries a bad signature, so all its later ones are held: nothing can be selected"""
    p = Pool(depth, SKELETON)
    for at, sig in zip((0, 1, 2, 4, 5, 6, 8), ("s_bit", "rx_ge_p", "s_bit255", "rx_plus1", "s_bit", "rx_ge_p", "s_bit255")):
        p.corrupt(at, sig)
    return p
