"""The reference and the cases of the witness-check tests (test_witness_check_cpu.py, test_gpu_witness_check.py,
test_gpu_cpp_witness_check.py).  The model states cstark_tx_witness_check on the plain pieces the other ledger tests already trust --
ledger_paths_cases.fold / leaf (the oracle's cso_rescue_merge), ledger_model.canonical / memory (Python integers mod p) and
sig_cases.reference (the oracle's SchnorrAir trace) -- one transfer at a time, with no early exit.  It shares nothing with the product.
The cases: the oracle's generated witnesses and their prefixes, the steered batches of ledger_scenarios.py through LedgerModel.apply,
and single-word mutations of every field of a witness.  Expectations are always the model's: a mutation that the model calls VALID is
kept and expected VALID."""
import functools

import numpy as np

import ledger_cases as LC
import ledger_model as LM
import ledger_paths_cases as PC
import ledger_scenarios as LS
import sig_cases as SC

P = LM.P
# cstark_witness_verdict (include/cstark.h): a transfer's verdict is the first that applies, in this order
(VALID, INDEX_RANGE, SELF_TRANSFER, SENDER_LEAF, SENDER_PATH, BALANCE, MIDDLE_ROOT, RECEIVER_LEAF, NEXT_ROOT, SIGNATURE) = range(10)
NAMES = ("VALID", "INDEX_RANGE", "SELF_TRANSFER", "SENDER_LEAF", "SENDER_PATH", "BALANCE", "MIDDLE_ROOT", "RECEIVER_LEAF", "NEXT_ROOT", "SIGNATURE")
DEPTHS = (1, 3, 15, 31)
SIZES = (1, 2, 3, 8)
FILL8, FILL64 = PC.FILL8, PC.FILL64
STATED = object()   # check(final_root=STATED): the witness's own final root


def _oracle():
    return LM._oracle()


def new_values(w, t):
    """(s_new, r_new) of transfer t: (pk, balance - delta, nonce + 1) and (pk, balance + delta, nonce), field arithmetic"""
    s_new, r_new = np.array(w.s_old_values[t], np.uint64), np.array(w.r_old_values[t], np.uint64)
    delta = LM.canonical(w.deltas[t])
    s_new[12] = LM.memory(LM.canonical(s_new[12]) - delta)
    s_new[13] = LM.memory(LM.canonical(s_new[13]) + 1)
    r_new[12] = LM.memory(LM.canonical(r_new[12]) + delta)
    return s_new, r_new


def messages(w):
    """[n_tx][28]: build_tx_message of every transfer's OWN row: sender's key, receiver's key, delta, the sender's old nonce, two zeros"""
    out = np.zeros((w.n_tx, 28), np.uint64)
    out[:, 0:12], out[:, 12:24], out[:, 24], out[:, 25] = w.s_old_values[:, :12], w.r_old_values[:, :12], w.deltas, w.s_old_values[:, 13]
    return out


_sig_cache = {}


def signature_verdicts(w):
    """cstark_sig_verdict of every transfer's signature over messages(w), by sig_cases.reference; one signature at a time, remembered by
    its bytes: the mutations of a witness share all but one"""
    msg, out = messages(w), np.zeros(w.n_tx, np.uint8)
    for t in range(w.n_tx):
        key = msg[t].tobytes() + np.asarray(w.sig_rx[t], np.uint64).tobytes() + np.asarray(w.sig_s[t], np.uint8).tobytes()
        if key not in _sig_cache:
            _sig_cache[key] = int(SC.reference(msg[t:t + 1], w.sig_rx[t:t + 1], w.sig_s[t:t + 1])[0][0])
        out[t] = _sig_cache[key]
    return out


def transfer_folds(w, t):
    """[4][7]: sender-old and receiver-new from the STATED leaf digests, sender-new and receiver-old from leaves hashed from values"""
    d, si, ri = w.depth, int(w.s_indices[t]), int(w.r_indices[t])
    s_new, _ = new_values(w, t)
    s_path, r_path = np.array(w.s_paths[t], np.uint64), np.array(w.r_paths[t], np.uint64)
    sender_old, receiver_new = PC.fold(si, s_path, d), PC.fold(ri, r_path, d)
    s_path[0], r_path[0] = PC.leaf(s_new), PC.leaf(w.r_old_values[t])
    return np.array([sender_old, PC.fold(si, s_path, d), PC.fold(ri, r_path, d), receiver_new], np.uint64)


def transfer_verdict(w, t, folds, final_root, sig_verdict=None):
    """every test of transfer t, then the first that fails.  final_root None: the last transfer has no NEXT_ROOT test;
    sig_verdict None: no signature test"""
    d, si, ri = w.depth, int(w.s_indices[t]), int(w.r_indices[t])
    _, r_new = new_values(w, t)
    next_root = w.initial_roots[t + 1] if t + 1 < w.n_tx else final_root
    failed = {
        INDEX_RANGE: si >= 1 << d or ri >= 1 << d,
        SELF_TRANSFER: si == ri,
        SENDER_LEAF: not np.array_equal(w.s_paths[t][0], PC.leaf(w.s_old_values[t])),
        SENDER_PATH: not np.array_equal(folds[0], w.initial_roots[t]),
        BALANCE: LM.canonical(w.deltas[t]) > LM.canonical(w.s_old_values[t][12]),
        MIDDLE_ROOT: not np.array_equal(folds[1], folds[2]),
        RECEIVER_LEAF: not np.array_equal(w.r_paths[t][0], PC.leaf(r_new)),
        NEXT_ROOT: next_root is not None and not np.array_equal(folds[3], np.asarray(next_root, np.uint64).reshape(7)),
        SIGNATURE: sig_verdict is not None and sig_verdict != SC.VALID,
    }
    return min([v for v, bad in failed.items() if bad], default=VALID)


class Expected:
    """the model's answer: verdicts [n_tx], folds [n_tx][4][7], final_root [7] (the last transfer's receiver-new fold), first_bad (-1:
    none), first_verdict, n_bad"""

    def __init__(self, verdicts, folds):
        self.verdicts, self.folds, self.final_root = verdicts, folds, folds[-1, 3].copy()
        bad = np.flatnonzero(verdicts)
        self.n_bad = len(bad)
        self.first_bad = int(bad[0]) if len(bad) else -1
        self.first_verdict = int(verdicts[bad[0]]) if len(bad) else VALID


def check(w, final_root=STATED, check_signatures=False):
    """-> Expected.  final_root: STATED (the witness's own, the host form), a root [7], or None (the resident form without one)"""
    final_root = w.final_root if final_root is STATED else final_root
    sig = signature_verdicts(w) if check_signatures else [None] * w.n_tx
    folds = np.array([transfer_folds(w, t) for t in range(w.n_tx)], np.uint64)
    verdicts = np.array([transfer_verdict(w, t, folds[t], final_root, sig[t]) for t in range(w.n_tx)], np.uint8)
    return Expected(verdicts, folds)


# ---- honest witnesses ------------------------------------------------------------------------------------------------------------------
def prefix(w, n):
    """the first n transfers of a witness: a witness whose final root is the root before transfer n"""
    O = _oracle()
    if n == w.n_tx:
        return w
    out = O.TxWitness(n, w.depth)
    for f in out.FIELDS:
        getattr(out, f)[...] = w.initial_roots[n] if f == "final_root" else getattr(w, f)[:n]
    return out


@functools.lru_cache(maxsize=None)
def generated(n_tx, depth):
    """the first n_tx transfers of the oracle's 8-transfer witness of `depth` (signed by its generator); shared, never written to"""
    w = prefix(LC.generated((8, depth, 40 + depth)), n_tx)
    for f in w.FIELDS:
        getattr(w, f).flags.writeable = False
    return w


def steered():
    """[(name, witness)]: every steered scenario the model applies: sibling and opposite-half pairs, deltas of 0 and of the whole
    balance, a nonce of p - 1 and a receiver balance that wraps past p (receiver_wraps_p), indices with bit 30 set at depth 31"""
    return [(sc.name, LS.expected(sc).witness) for sc in LS.SCENARIOS + LS.ACCEPTED]


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
def _copy(w):
    out = w.copy()
    for f in out.FIELDS:
        getattr(out, f).flags.writeable = True
    return out


def _bump(a, at):
    a[at] = PC.bump(a[at])


def mutations(w, t):
    """[(name, witness)]: w with ONE word changed (the last two: two words), at transfer t where the field has one per transfer: every
    field of the witness, the leaf, the first and the last sibling of both paths, indices out of range, equal and moved, a delta one
    above the balance, words of p - 1, both halves of the signature"""
    d, out = w.depth, []

    def add(name, change):
        m = _copy(w)
        change(m)
        out.append((name, m))

    add("initial_root", lambda m: _bump(m.initial_roots, (t, 0)))
    add("initial_root_last_word", lambda m: _bump(m.initial_roots, (t, 6)))
    if t + 1 < w.n_tx:
        add("next_initial_root", lambda m: _bump(m.initial_roots, (t + 1, 3)))
    add("final_root", lambda m: _bump(m.final_root, 2))
    add("final_root_p_minus_1", lambda m: m.final_root.__setitem__(6, P - 1))
    add("s_key", lambda m: _bump(m.s_old_values, (t, 0)))
    add("s_balance", lambda m: _bump(m.s_old_values, (t, 12)))
    add("s_nonce", lambda m: _bump(m.s_old_values, (t, 13)))
    add("s_nonce_p_minus_1", lambda m: m.s_old_values.__setitem__((t, 13), P - 1))
    add("r_key", lambda m: _bump(m.r_old_values, (t, 11)))
    add("r_balance", lambda m: _bump(m.r_old_values, (t, 12)))
    add("r_nonce", lambda m: _bump(m.r_old_values, (t, 13)))
    add("s_index_range", lambda m: m.s_indices.__setitem__(t, 1 << d))
    add("r_index_range", lambda m: m.r_indices.__setitem__(t, 1 << d))
    add("r_index_bit63", lambda m: m.r_indices.__setitem__(t, int(m.r_indices[t]) | 1 << 63))
    add("self_transfer", lambda m: m.s_indices.__setitem__(t, m.r_indices[t]))
    add("s_index_low_bit", lambda m: m.s_indices.__setitem__(t, int(m.s_indices[t]) ^ 1))
    add("r_index_top_bit", lambda m: m.r_indices.__setitem__(t, int(m.r_indices[t]) ^ 1 << (d - 1)))
    add("s_leaf", lambda m: _bump(m.s_paths, (t, 0, 0)))
    add("s_first_sibling", lambda m: _bump(m.s_paths, (t, 1, 6)))
    add("s_last_sibling", lambda m: _bump(m.s_paths, (t, d, 3)))
    add("s_sibling_p_minus_1", lambda m: m.s_paths.__setitem__((t, d, 0), P - 1))
    add("r_leaf", lambda m: _bump(m.r_paths, (t, 0, 6)))
    add("r_first_sibling", lambda m: _bump(m.r_paths, (t, 1, 0)))
    add("r_last_sibling", lambda m: _bump(m.r_paths, (t, d, 5)))
    add("delta_plus_1", lambda m: _bump(m.deltas, t))
    add("delta_zero", lambda m: m.deltas.__setitem__(t, 0))
    add("delta_balance_plus_1", lambda m: m.deltas.__setitem__(t, LM.memory(LM.canonical(m.s_old_values[t][12]) + 1)))
    add("delta_p_minus_1", lambda m: m.deltas.__setitem__(t, LM.memory(P - 1)))
    add("sig_rx", lambda m: _bump(m.sig_rx, (t, 5)))
    add("sig_s_byte", lambda m: m.sig_s.__setitem__((t, 17), m.sig_s[t, 17] ^ 0x10))
    add("sig_s_bit255", lambda m: m.sig_s.__setitem__((t, 31), m.sig_s[t, 31] | 0x80))
    add("path_and_signature", lambda m: (_bump(m.s_paths, (t, 1, 2)), m.sig_s.__setitem__((t, 0), m.sig_s[t, 0] ^ 1)))
    add("receiver_leaf_and_signature", lambda m: (_bump(m.r_paths, (t, 0, 1)), _bump(m.sig_rx, (t, 0))))
    return out


@functools.lru_cache(maxsize=None)
def mutation_set(depth):
    """[(name, witness, Expected with the signature test)]: the mutations of the inner transfer of the generated 3-transfer witness of
    `depth`; computed once and shared"""
    return [(name, m, check(m, check_signatures=True)) for name, m in mutations(generated(3, depth), 1)]
