"""CPU model of the unreduced arithmetic the device kernels rely on, and the hand-derived bounds behind it.

fp_mul_lazy (csrc/fp.cuh) is restated word for word in numpy: every 64-bit sum is checked for a carry out and the 32-bit sum c for a
wrap, so the bounds its comments state are checked here on the very words the device computes.  The same model runs the 74-product
inverse S-box chain of fp_inv_sbox over 2^20 inputs (its 1.78 p ceiling) and supplies tests/test_gpu_extremes.py with the inputs that
drive the chain highest.  The section sums of csrc/rounds_mfma.hip (28 centred products riding on 2p 2^64) are bounded in Python
integers.  No GPU needed."""
import random

import numpy as np

P = 2**62 + 2**56 + 2**55 + 1
P1 = 0x41800000
K = P1 + 1
M32 = 2**32 - 1
R_INV = pow(2**64, -1, P)
HALF_P = (P - 1) // 2
X0 = 0x0080808080808080          # byte offset of the matrix-core operands (mds_mfma.cuh)
INV_ALPHA = 3146514939656186539
B1_LIMIT = 2**32 - 1 - K         # largest high word of the second factor for which c = (w >> 32) + K cannot wrap: 0xBE7FFFFE


def _add(a, b, flag):
    s = a + b
    flag |= s < a
    return s, flag


def mul_lazy(a, b):
    """fp_mul_lazy on uint64 arrays, step for step.  Returns (result, wrapped): wrapped marks any sum that left its register."""
    a = np.asarray(a, np.uint64)
    b = np.asarray(b, np.uint64)
    m32, s32 = np.uint64(M32), np.uint64(32)
    a0, a1, b0, b1 = a & m32, a >> s32, b & m32, b >> s32
    wr = np.zeros(np.broadcast(a, b).shape, bool)
    t = a0 * b0
    s = (t >> s32) + np.uint64(K)                               # < 2^33: never wraps
    u, wr = _add(a1 * b0, s, wr)
    v, wr = _add((~t & m32) * np.uint64(P1), u, wr)
    w, wr = _add(a0 * b1, v & m32, wr)
    c = (w >> s32) + np.uint64(K)
    wr |= c > m32                                                # the 32-bit add of line 78
    c &= m32
    x, wr = _add(a1 * b1, c, wr)
    x, wr = _add(v >> s32, x, wr)
    r, wr = _add((~w & m32) * np.uint64(P1), x, wr)
    return r, wr


def mul_lazy_int(a, b):
    """The same word steps in Python integers (an independent transliteration), None when a sum wraps."""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    t = a0 * b0
    u = a1 * b0 + (t >> 32) + K
    v = ((~t) & M32) * P1 + u
    w = a0 * b1 + (v & M32)
    c = (w >> 32) + K
    x = a1 * b1 + c + (v >> 32)
    r = ((~w) & M32) * P1 + x
    if max(u, v, w, x, r) >= 2**64 or c > M32:
        return None
    return r


def _reduce_once(r):
    return np.where(r >= np.uint64(P), r - np.uint64(P), r)


def inv_sbox_chain(x):
    """fp_inv_sbox's chain on the model: (result, largest unreduced value of every lane, any wrap).  Every operand of every product
    and every value handed to a single conditional subtraction enters the maximum."""
    x = np.asarray(x, np.uint64)
    hi = x.copy()
    wr = np.zeros(x.shape, bool)

    def mul(a, b):
        nonlocal hi, wr
        r, w = mul_lazy(a, b)
        wr |= w
        hi = np.maximum(hi, r)
        return r

    x2 = _reduce_once(mul(x, x))
    x3 = _reduce_once(mul(x2, x))
    x5 = mul(x3, x2)
    x10 = mul(x5, x5)
    x21 = mul(mul(x10, x10), x)
    x42 = _reduce_once(mul(x21, x21))
    r = mul(x42, x)
    for _ in range(9):
        for _ in range(6):
            r = mul(r, r)
        r = mul(r, x42)
    r = mul(r, r)
    r = mul(r, r)
    return _reduce_once(mul(r, x3)), hi, wr


def inv_sbox_candidates(n=1 << 20, seed=2024):
    """2^20 inputs: the field's edges, structured words and uniform ones"""
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, P - 1, P - 2, HALF_P, HALF_P + 1, 2**32 - 1, 2**32, 2**62, P - 2**32, 0x3b7ffffffffffffd]
    xs = rng.integers(0, P, size=n, dtype=np.uint64)
    xs[:len(edge)] = np.array(edge, np.uint64)
    return xs


def inv_sbox_extremes(k=2048, n=1 << 20):
    """the k inputs among the candidates whose lazy chain climbs highest"""
    xs = inv_sbox_candidates(n)
    _, hi, _ = inv_sbox_chain(xs)
    order = np.argsort(hi, kind="stable")[::-1][:k]
    return xs[order], hi[order]


# ---- fp_mul_lazy ----------------------------------------------------------------------------------------------------------------

def _lazy_pairs():
    rng = random.Random(5)
    big = [P, P + 1, P + 2, P + 2**32, 2 * P - 1, 2 * P - 2, 2 * P - 2**32, (3 * P) // 2, P + HALF_P]
    big += [rng.randrange(P, 2 * P) for _ in range(200)]
    return [(a, b) for a in big for b in big]


def test_model_equals_the_integer_transliteration():
    rng = random.Random(11)
    words = [0, 1, M32, 2**32, 2**64 - 1, P - 1, P, 2 * P - 1, (B1_LIMIT << 32) | M32, ((B1_LIMIT + 1) << 32) | M32]
    words += [rng.randrange(2**64) for _ in range(300)]
    a = np.array([x for x in words for _ in words], np.uint64)
    b = np.array([y for _ in words for y in words], np.uint64)
    r, wr = mul_lazy(a, b)
    for x, y, got, w in zip(a.tolist(), b.tolist(), r.tolist(), wr.tolist()):
        want = mul_lazy_int(x, y)
        assert w == (want is None), (hex(x), hex(y))
        if want is not None:
            assert got == want, (hex(x), hex(y))


def test_lazy_product_for_both_factors_in_p_2p():
    """what fp_inv_sbox's callers rely on, for a, b in [p, 2p): no sum wraps, r = a b 2^-64 (mod p) and r <= a b / 2^64 + p + p / 2^32.
    The extra p / 2^32 is real: REDC's word quotients lie in [1, 2^32] (q = 2^32 for a zero low word), so q reaches 2^64 + 2^32, and
    a = b = 2p - 2 (zero low words) lands ON a b / 2^64 + p, which fp.cuh once stated as a strict bound."""
    pairs = _lazy_pairs()
    a = np.array([x for x, _ in pairs], np.uint64)
    b = np.array([y for _, y in pairs], np.uint64)
    r, wr = mul_lazy(a, b)
    assert not wr.any()
    for x, y, got in zip(a.tolist(), b.tolist(), r.tolist()):
        assert got % P == x * y * R_INV % P
        assert got * 2**64 <= x * y + P * (2**64 + 2**32)
    r, _ = mul_lazy(np.uint64(2 * P - 2), np.uint64(2 * P - 2))
    assert int(r) * 2**64 >= (2 * P - 2)**2 + P * 2**64          # q = 2^64 exactly: the strict bound fails


def test_second_factor_high_word_limit_is_0xBE7FFFFE():
    """c = (w >> 32) + K is a 32-bit sum.  w = a0 b1 + (v mod 2^32) < 2^32 (b1 + 1), so w >> 32 <= b1 and c cannot wrap for
    b1 <= 0xBE7FFFFE; at b1 = 0xBE7FFFFF it wraps once a0 and the low word of v are large.  3 * 2^30 (the old comment) is past it."""
    assert B1_LIMIT == 0xBE7FFFFE and B1_LIMIT < 3 * 2**30
    assert ((M32 * B1_LIMIT + M32) >> 32) + K <= M32
    assert ((M32 * (B1_LIMIT + 1) + M32) >> 32) + K > M32
    assert (2 * P - 1) >> 32 == 0x83000000 < B1_LIMIT      # every second factor below 2p is far inside
    rng = np.random.default_rng(3)
    a = (rng.integers(0, 2**31, size=1 << 16, dtype=np.uint64) << np.uint64(32)) | np.uint64(M32)
    lows = rng.integers(0, 2**32, size=a.size, dtype=np.uint64)
    _, wr_ok = mul_lazy(a, (np.uint64(B1_LIMIT) << np.uint64(32)) | lows)
    assert not wr_ok.any()
    _, wr_bad = mul_lazy(a, (np.uint64(B1_LIMIT + 1) << np.uint64(32)) | lows)
    assert wr_bad.any()


def test_inverse_sbox_chain_stays_below_its_ceiling():
    """fp_inv_sbox on unreduced values over 2^20 inputs: no sum wraps, every value stays below 1.78 p (the documented ceiling, so
    below 2p where the lazy product's bound holds), and the chain computes x^INV_ALPHA"""
    xs = inv_sbox_candidates()
    res, hi, wr = inv_sbox_chain(xs)
    assert not wr.any()
    top = int(hi.max())
    assert top < 1.78 * P, top / P
    assert top > 1.5 * P                                # the candidates climb well past p (1.558 p with this seed)
    assert (res < np.uint64(P)).all()
    rng = random.Random(4)
    for i in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11] + [rng.randrange(xs.size) for _ in range(200)] + [int(np.argmax(hi))]:
        x = int(xs[i])
        # memory form: x = X R, result = X^INV_ALPHA R
        assert int(res[i]) == pow(x * R_INV % P, INV_ALPHA, P) * 2**64 % P, hex(x)


def test_extreme_inputs_are_the_chains_highest():
    xs, hi = inv_sbox_extremes(k=64, n=1 << 16)
    assert (np.diff(hi.astype(np.float64)) <= 0).all() and (xs < np.uint64(P)).all()


# ---- the matrix-core section sums (rounds_mfma.hip) -----------------------------------------------------------------------------

def section_value(coeffs, cubes):
    """The integer handed to the Montgomery reduction for one section: coefficients centred into (-p/2, p/2], operands
    cube - (p-1)/2, both with the byte offset X0 of the operand removed again by the row constant, plus 2p 2^64.
    Returns (value, the row constant part kc) in Python integers."""
    cc = [c - P if c > HALF_P else c for c in coeffs]
    g = sum(c * (x - HALF_P - X0) for c, x in zip(cc, cubes))
    kc = (X0 + HALF_P) * (sum(coeffs) % P) * 1 % P
    return g + kc + 2 * P * 2**64, kc


def test_section_sums_fit_their_128_bit_accumulator():
    """|sum of 28 centred products| <= 28 (p-1)/2 ((p-1)/2 + X0) = 7.11 p^2; around 2p 2^64 it stays inside [0, 2^128) with about 2 %
    headroom at the top; around p 2^64 it would not stay non-negative.  One fold then brings the high word below 2p."""
    gmax = 28 * HALF_P * (HALF_P + X0)
    assert 7.1 * P * P < gmax < 7.12 * P * P
    assert 2 * P * 2**64 - gmax > 0
    assert 2 * P * 2**64 + (P - 1) + gmax < 2**128
    assert (2**128 - (2 * P * 2**64 + (P - 1) + gmax)) / 2**128 > 0.02
    assert P * 2**64 - gmax < 0                       # the offset must be 2p 2^64: p 2^64 goes negative at the extremes
    assert (2**128 - 1) >> 64 < 4 * P                 # acc_fold's single subtraction of 2p suffices
    # the extremes are reached by concrete coefficient / operand pairs and the value is congruent to the plain dot product
    for coeffs, cubes in (([HALF_P + 1] * 28, [0] * 28), ([HALF_P] * 28, [0] * 28), ([HALF_P] * 28, [P - 1] * 28)):
        v, _ = section_value(coeffs, cubes)
        assert 0 <= v < 2**128
        assert v % P == sum(c * x for c, x in zip(coeffs, cubes)) % P
    vmax, _ = section_value([HALF_P + 1] * 28, [0] * 28)
    assert vmax > 0.97 * 2**128
