"""References and builders of the signature-check tests (test_sig_reference_cpu.py, test_gpu_sig_check.py, test_gpu_ledger_checked.py,
test_gpu_cpp_sigcheck.py).  The reference for every value is the oracle's SchnorrAir trace: registers 0..5 of row 511 of signature i's
block hold the affine x of s*G + h*P that verify_signature (src/schnorr/mod.rs:220-245) compares with R.x, registers 12..17 the Z the
complete addition left (zero: the point at infinity); the oracle's curve equation gives the key verdict."""
import functools
import os
import subprocess

import numpy as np

import ledger_cases as LC

P = 2**62 + 2**56 + 2**55 + 1
VALID, MISMATCH, KEY_NOT_ON_CURVE, SCALAR_RANGE = 0, 1, 2, 3   # cstark_sig_verdict
SIGNATURE = 5                                                  # cstark_ledger_reason

# one change to signature j of a batch; every one of them must turn a valid signature into MISMATCH
PERTURBATIONS = ("s_bit0", "s_bit254", "rx_word0", "rx_word5", "msg12", "msg24", "msg25", "msg26", "msg27", "other_key")


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def generated(count, seed=0x5EED):
    """(messages [count][28], sig_rx [count][6], sig_s [count][32]) of the oracle's generator; computed once, never written to"""
    w = _oracle().SchnorrWitness.generate(count, seed)
    arrays = (w.messages, w.sig_rx, w.sig_s)
    for a in arrays:
        a.flags.writeable = False
    return arrays


def reference(messages, sig_rx, sig_s):
    """-> (verdicts uint8 [count], x uint64 [count][6]) from the oracle's SchnorrAir trace of these signatures"""
    O = _oracle()
    messages = np.ascontiguousarray(messages, np.uint64).reshape(-1, 28)
    n = messages.shape[0]
    w = O.SchnorrWitness(n)
    w.messages[...] = messages
    w.sig_rx[...] = np.asarray(sig_rx, np.uint64).reshape(n, 6)
    w.sig_s[...] = np.asarray(sig_s, np.uint8).reshape(n, 32)
    trace = O.schnorr_build_trace(w)
    last = trace[:, 511::512]
    x, z = np.ascontiguousarray(last[0:6].T), last[12:18].T
    verdicts = np.zeros(n, np.uint8)
    for i in range(n):
        if w.sig_s[i, 31] >> 7:
            verdicts[i] = SCALAR_RANGE
        elif O.lib().cso_ecc_on_curve_affine(O._p(np.ascontiguousarray(w.messages[i, :12]))) != 1:
            verdicts[i] = KEY_NOT_ON_CURVE
        elif not z[i].any() or not np.array_equal(x[i], w.sig_rx[i]):
            verdicts[i] = MISMATCH
    return verdicts, x


@functools.lru_cache(maxsize=None)
def generated_reference(count, seed=0x5EED):
    v, x = reference(*generated(count, seed))
    v.flags.writeable = False
    x.flags.writeable = False
    return v, x


def _bump(word):
    """another reduced field element"""
    return np.uint64((int(word) + 1) % P)


def perturbed(arrays, j, kind):
    """copies of (messages, sig_rx, sig_s) with signature j changed in one way"""
    m, rx, s = (a.copy() for a in arrays)
    if kind == "s_bit0":
        s[j, 0] ^= 1
    elif kind == "s_bit254":
        s[j, 31] ^= 0x40
    elif kind.startswith("rx_word"):
        k = int(kind[7:])
        rx[j, k] = _bump(rx[j, k])
    elif kind.startswith("msg"):
        k = int(kind[3:])
        m[j, k] = _bump(m[j, k])
    elif kind == "other_key":
        m[j, :12] = m[(j + 1) % len(m), :12]
    else:
        raise ValueError(kind)
    return m, rx, s


def off_curve(arrays, j):
    """signature j's key with one word changed"""
    m, rx, s = (a.copy() for a in arrays)
    m[j, 3] = _bump(m[j, 3])
    return m, rx, s


def scalar_extremes(arrays):
    """a batch of five: s = 0, 1, 2^255 - 1, 2^254 in place of the first four scalars, and the fifth, valid, with bit 255 set"""
    m, rx, s = (a[:5].copy() for a in arrays)
    for i, value in enumerate((0, 1, 2**255 - 1, 2**254)):
        s[i] = np.frombuffer(value.to_bytes(32, "little"), np.uint8)
    s[4, 31] |= 0x80
    return m, rx, s


def tx_messages(w, hi=None):
    """The messages the transfers [0, hi) of a transaction witness sign (build_tx_message, src/lib.rs:467-481), from a walk of its own
    over the accounts: sender's key, receiver's key, delta, the sender's nonce as the transfers before leave it, two zeros.  Only the
    initial accounts, indices and deltas are read (the old values of the witness are what the walk must reproduce)."""
    O = _oracle()
    hi = w.n_tx if hi is None else hi
    one = O.to_mont(np.array([1], np.uint64))[0]
    indices, values = LC.initial_accounts(w)
    state = {int(i): v.copy() for i, v in zip(indices, values)}
    out = np.zeros((hi, 28), np.uint64)
    for t in range(hi):
        sv, rv, delta = state[int(w.s_indices[t])], state[int(w.r_indices[t])], w.deltas[t]
        out[t, 0:12], out[t, 12:24], out[t, 24], out[t, 25] = sv[:12], rv[:12], delta, sv[13]
        d = np.array([delta], np.uint64)
        sv[12] = O.fp_sub(sv[12:13].copy(), d)[0]
        sv[13] = O.fp_add(sv[13:14].copy(), np.array([one], np.uint64))[0]
        rv[12] = O.fp_add(rv[12:13].copy(), d)[0]
    return out


def nonce_moved(w):
    """transfers whose sender signs another nonce than the one its account had before the batch"""
    first = {}
    moved = []
    for t in range(w.n_tx):
        for idx, val in ((int(w.s_indices[t]), w.s_old_values[t]), (int(w.r_indices[t]), w.r_old_values[t])):
            first.setdefault(idx, int(val[13]))
        if int(w.s_old_values[t, 13]) != first[int(w.s_indices[t])]:
            moved.append(t)
    return moved


def transfers(w, lo=0, hi=None):
    return tuple(getattr(w, f)[lo:hi] for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))


def build_messages_checker(directory, sanitize=True):
    """tests/cpp/ledger_messages_check.cpp as a stand-alone program: with AddressSanitizer and UBSan for the tests, -O2 for timing"""
    exe = os.path.join(str(directory), "ledger_messages_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(LC.ROOT, "tests", "cpp", "ledger_messages_check.cpp")])
    return exe


def write_messages_case(path, w, batch=None, messages=None, refusal=None):
    """A case as tests/cpp/ledger_messages_check.cpp reads it.  batch: (s_indices, r_indices, deltas, sig_rx, sig_s) when they are not
    the witness's own; messages: those the plan must build (all of them, or the ones before `refusal` = (refused_at, reason))"""
    s, r, d, rx, ss = transfers(w) if batch is None else batch
    indices, values = LC.initial_accounts(w)
    messages = tx_messages(w) if messages is None else messages
    n_msg = len(messages)
    head = np.array([w.depth, len(indices), len(s), n_msg] + ([2**64 - 1, 0] if refusal is None else list(refusal)), np.uint64)
    with open(path, "wb") as f:
        for a in (head, indices, values, s, r, d, messages, rx[:n_msg]):
            f.write(np.ascontiguousarray(a, "<u8").tobytes())
        f.write(np.ascontiguousarray(ss[:n_msg], np.uint8).tobytes())


def flipped(w, j):
    """the transfers of w with one bit of transfer j's scalar flipped"""
    s, r, d, rx, ss = (a.copy() for a in transfers(w))
    ss[j, 0] ^= 1
    return s, r, d, rx, ss
