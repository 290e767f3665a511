"""The reference signer of the signing tests (test_sign_reference_cpu.py, test_gpu_sign_nonces.py, test_gpu_sign.py,
test_gpu_ledger_sign.py, test_gpu_cpp_sign.py), from the oracle and Python integers only: R = r*G by the oracle's double-and-add
(cso_ecc_scalar_mul_affine over the five limbs of the nonce), h by cso_schnorr_hash_message read as a 4-limb integer, s = r - sk*h and
the status by integer arithmetic, r = 0 handled apart as INFINITY (the oracle would invert zero), the nonce stream of the seeded signer
restated here, and the first-accepted rule."""
import ctypes as C
import functools
import random

import numpy as np

import sig_cases as SC

P = SC.P
OK, NEGATIVE, RANGE, INFINITY, EXHAUSTED = 0, 1, 2, 3, 4     # cstark_sign_status
MAX_SECRET = 255
KEY = 7                                                     # cstark_ledger_reason
M64 = 2**64 - 1
# GENERATOR in memory form (src/utils/ecc.rs:23-36), as tests/test_oracle_field.py states it
GEN_RAW = [0xf6798582c92ece1, 0x2b7c30a4c7d886c0, 0x1269cdae98dc2fd0, 0x11b78ef6c71c6132, 0x3ac2244dfc47537, 0x36dfeea4b9051daf,
           0x334807e450d55e2f, 0x200a54d42b84bd17, 0x271af7bb20ab32e1, 0x3df7b90927efc7ec, 0xab8bbf4a53af6a0, 0xe13dca26b2ac6ab]


def _oracle():
    return SC._oracle()


def limbs(r, n=5):
    assert 0 <= r < 2**(64 * n)
    return np.array([(r >> (64 * i)) & M64 for i in range(n)], np.uint64)


def nonce_array(rs):
    return np.array([limbs(r) for r in rs], np.uint64).reshape(-1, 5)


@functools.lru_cache(maxsize=None)
def _point(r):
    O = _oracle()
    out = np.zeros(12, np.uint64)
    O.lib().cso_ecc_scalar_mul_affine(O._p(limbs(r)), C.c_uint(5), O._p(np.array(GEN_RAW, np.uint64)), O._p(out))
    out.flags.writeable = False
    return out


def scalar_mul(r):
    """r*G as [12] affine words in memory form, for 0 < r < 2^320"""
    assert r > 0
    return _point(int(r))


def public_keys(secrets):
    return np.array([scalar_mul(int(sk)) for sk in secrets], np.uint64).reshape(-1, 12)


def on_curve(point12):
    O = _oracle()
    return O.lib().cso_ecc_on_curve_affine(O._p(np.ascontiguousarray(point12, np.uint64))) == 1


def hash_to_int(rx, message):
    O = _oracle()
    out = np.zeros(7, np.uint64)
    O.lib().cso_schnorr_hash_message(O._p(np.ascontiguousarray(rx, np.uint64)), O._p(np.ascontiguousarray(message, np.uint64)), O._p(out))
    return sum(int(c) << (64 * i) for i, c in enumerate(O.from_mont(out[:4].copy())))


def attempt(message, sk, r):
    """one signing attempt -> (sig_rx uint64 [6], sig_s uint8 [32], status); every output is defined whatever the status"""
    sk, r = int(sk), int(r)
    assert 1 <= sk <= MAX_SECRET and 0 <= r < 2**264
    rx = np.zeros(6, np.uint64) if r == 0 else scalar_mul(r)[:6].copy()
    d = r - sk * hash_to_int(rx, message)
    status = INFINITY if r == 0 else NEGATIVE if d < 0 else RANGE if d >= 2**255 else OK
    s = np.frombuffer((d & (2**256 - 1)).to_bytes(32, "little"), np.uint8).copy()
    return rx, s, status


def attempts(messages, secrets, nonces):
    """the reference of schnorr_sign_nonces: nonces are Python integers -> (sig_rx [n][6], sig_s [n][32], status [n])"""
    got = [attempt(m, sk, r) for m, sk, r in zip(messages, secrets, nonces)]
    return (np.array([g[0] for g in got], np.uint64).reshape(-1, 6), np.array([g[1] for g in got], np.uint8).reshape(-1, 32),
            np.array([g[2] for g in got], np.uint8))


# ---- the seeded signer ----
def _splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def nonce_stream(seed, t, sk):
    """the nonces of signature t under `seed`, attempt by attempt (Python integers, below (sk + 2) * 2^254)"""
    state = (seed ^ (0xD1B54A32D192ED03 * (t + 1))) & M64
    while True:
        out = []
        for _ in range(5):
            state, z = _splitmix64(state)
            out.append(z)
        r3 = out[3] & (2**62 - 1)
        top = r3 + ((out[4] % (sk + 2)) << 62)
        yield out[0] | (out[1] << 64) | (out[2] << 128) | (top << 192)


class Signed:
    """the reference of schnorr_sign: the first accepted attempt of every signature, or EXHAUSTED with zero outputs"""

    def __init__(self, messages, secrets, seed, max_attempts):
        n = len(secrets)
        self.sig_rx, self.sig_s = np.zeros((n, 6), np.uint64), np.zeros((n, 32), np.uint8)
        self.attempts, self.status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self.rejected = []          # (signature, sig_rx, sig_s, status) of every attempt ahead of an accepted one, or of an exhausted signature
        for t in range(n):
            stream = nonce_stream(seed, t, int(secrets[t]))
            self.status[t], self.attempts[t] = EXHAUSTED, max_attempts
            for a in range(max_attempts):
                rx, s, status = attempt(messages[t], secrets[t], next(stream))
                if status == OK:
                    self.sig_rx[t], self.sig_s[t], self.status[t], self.attempts[t] = rx, s, OK, a + 1
                    break
                self.rejected.append((t, rx, s, status))
        for a in (self.sig_rx, self.sig_s, self.attempts, self.status):
            a.flags.writeable = False

    @property
    def total_attempts(self):
        return int(self.attempts.sum())


def payload_messages(secrets, seed):
    """messages [n][28] in memory form: the public key of secrets[i], then 16 reduced words from the seed (src/schnorr/mod.rs:94-99)"""
    rng = random.Random(seed)
    n = len(secrets)
    m = np.zeros((n, 28), np.uint64)
    m[:, :12] = public_keys(secrets)
    m[:, 12:] = _oracle().to_mont(np.array([[rng.randrange(P) for _ in range(16)] for _ in range(n)], np.uint64)).reshape(n, 16)
    return m


# the batches the GPU tests sign: computed once per process and shared, never written to
SEED = 0x51C4A7
SMALL_KEYS = tuple(1 + i % 8 for i in range(24))     # keys 1..8, three signatures each


@functools.lru_cache(maxsize=None)
def small_batch():
    sk = np.array(SMALL_KEYS, np.uint64)
    m = payload_messages(sk, 0xBA7C4)
    m.flags.writeable = False
    sk.flags.writeable = False
    return m, sk


@functools.lru_cache(maxsize=None)
def small_signed(max_attempts):
    return Signed(*small_batch(), SEED, max_attempts)
