"""GPU parity for the stage between the constraint commitment and FRI: the out-of-domain frame (csrc/deep.hip k_poly_eval_*, csrc/ext.hip
k_poly_eval_ext_*, k_ood_recombine) and the DEEP composition (k_deep, k_deep_ext, k_deep_ext_consts), over the base field and both
extensions, through the host-argument entry points and through the device-resident forms the device channel uses.  The inputs are the
ones a whole proof never presents: zero, p - 1 words, embedded base-field points, the adjoined root, sparse and saturated columns,
every segment count, every remainder of the fold-every-4 loop.  Every comparison is bit-exact: against the oracle at every shape, and
against Python integers (the e_* tuples of oracle/verifier.py) at the small ones."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2**62 + 2**56 + 2**55 + 1
R = 2**64
R_INV = pow(R, -1, P)


def mont(x):
    return x * R % P


def canon(w):
    return int(w) * R_INV % P


EXT = [0, P - 1, (P - 1) // 2, (P + 1) // 2, mont(1)]          # the word constants of test_gpu_extremes.py


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _V():
    from oracle import verifier as V
    return V


# ---- the extension in Python integers: tuples of m canonical values (m = 1: the base field) -------------------------------------------
def x_mul(x, y):
    return (x[0] * y[0] % P,) if len(x) == 1 else _V().e_mul(x, y)


def x_inv(x):
    return (pow(x[0], -1, P),) if len(x) == 1 else _V().e_inv(x)


def x_add(x, y):
    return tuple((a + b) % P for a, b in zip(x, y))


def x_sub(x, y):
    return tuple((a - b) % P for a, b in zip(x, y))


def x_scale(x, s):
    return tuple(a * s % P for a in x)


def x_base(v, m):
    return (v % P,) + (0,) * (m - 1)


def x_pow(x, e):
    r = x_base(1, len(x))
    while e:
        if e & 1:
            r = x_mul(r, x)
        x = x_mul(x, x)
        e >>= 1
    return r


def tup(words):
    return tuple(canon(w) for w in words)


def words(t):
    return [mont(v) for v in t]


def canon_list(oracle, a):
    return [int(v) for v in oracle.from_mont(np.ascontiguousarray(a, np.uint64).reshape(-1))]


def horner(canon_coeffs, z):
    """sum_k c_k z^k for base coefficients (canonical integers) at the point z (tuple) by a plain Horner chain"""
    m = len(z)
    if m == 1:
        acc, z0 = 0, z[0]
        for c in reversed(canon_coeffs):
            acc = (acc * z0 + c) % P
        return (acc,)
    acc = (0,) * m
    for c in reversed(canon_coeffs):
        acc = x_mul(acc, z)
        acc = ((acc[0] + c) % P,) + acc[1:]
    return acc


# ---- A. point evaluation -----------------------------------------------------------------------------------------------------------
SIZES = [6, 8, 9, 14, 15, 17]   # a short column with a guarded tail | one coefficient per lane | two per lane | 1, 2 and 8 segments
N_COLUMN_KINDS = 6


def column_sets(log_n):
    """(width, kind of the first column): every column kind is reached at every width"""
    if log_n == 17:
        return [(2, 0), (2, 2), (2, 4)]
    return [(1, s) for s in range(N_COLUMN_KINDS)] + [(3, 0), (3, 3), (94, 0)]


SATURATED, GAPPED = 1, 5


def make_column(oracle, kind, n, seed):
    col = np.zeros(n, np.uint64)
    if kind == 0:
        col = oracle.random_elements(n, seed)
    elif kind == 1:
        col[:] = P - 1
    elif kind == 2:
        col[1::2] = P - 1
    elif kind == 3:
        col[n - 1] = EXT[3]
    elif kind == 4:
        col[16384 % n] = P - 1        # the first coefficient of the second segment (index 0 of a column that has one segment)
    else:
        col[:] = P - 1                # saturated but for the ninth coefficient of every lane (test_lazy_sum_model_of_the_extension_evaluation)
        col[8 * 256:9 * 256] = 0
    return col


class Tables:
    """the coefficient tables of section A, built once per size and shared by its tests (host and device copies, never written)"""

    def __init__(self, oracle, backend):
        self.oracle, self.backend, self.cache = oracle, backend, {}

    def __call__(self, log_n):
        if log_n not in self.cache:
            n, out = 1 << log_n, []
            for width, first in column_sets(log_n):
                co = np.stack([make_column(self.oracle, (first + i) % N_COLUMN_KINDS, n, 1000 * log_n + 10 * i + first) for i in range(width)])
                out.append((co, self.backend.from_numpy_u64(co), first))
            self.cache[log_n] = out
        return self.cache[log_n]


@pytest.fixture(scope="module")
def tabs(oracle, backend):
    return Tables(oracle, backend)


def base_point_kinds(oracle, log_n):
    """memory-form words: random, 0, 1, the word p - 1, -1, a primitive 256th root of unity, w_n"""
    return [int(oracle.random_elements(1, 4242 + log_n)[0]), 0, mont(1), P - 1, mont(P - 1), oracle.root_of_unity(8), oracle.root_of_unity(log_n)]


def base_points(oracle, log_n, npts):
    kinds = base_point_kinds(oracle, log_n)
    pts = [kinds[(npts + i) % len(kinds)] for i in range(min(npts, len(kinds)))]
    return pts + [int(v) for v in oracle.random_elements(npts - len(pts), 77 * npts + log_n)]


def ext_points(oracle, log_n, m):
    """m-tuples of words: a random element, the embedded base kinds, the adjoined root, every component p - 1, zero"""
    pad = [0] * (m - 1)
    pts = [[int(v) for v in oracle.random_elements(m, 99 + log_n + m)]]
    pts += [[w] + pad for w in base_point_kinds(oracle, log_n) if w != 0]
    pts += [[0, mont(1)] + [0] * (m - 2), [P - 1] * m, [0] * m, [P - 1] + pad[:-1] + [EXT[3]]]
    return pts


@pytest.mark.parametrize("log_n", SIZES)
def test_point_evaluation_base(oracle, backend, tabs, log_n):
    """cstark_evaluate_polys_at for 1, 2, 3, 5 and 16 points (the single-point template, an odd count, the ABI's maximum), every point
    compared with the oracle; Python-integer Horner for all of them at n <= 512 and for the saturated column at 2^15"""
    for co, d_co, first in tabs(log_n):
        for npts in (1, 2, 3, 5, 16):
            pts = base_points(oracle, log_n, npts)
            got = backend.evaluate_polys_at(d_co, pts)
            assert got.shape == (npts, co.shape[0])
            assert (got == oracle.evaluate_polys_at(co, pts)).all(), (co.shape, npts)
            ints = log_n <= 9 or (log_n == 15 and co.shape[0] == 1 and first == SATURATED)
            if ints and npts == 16:
                for c in range(co.shape[0]):
                    cc = canon_list(oracle, co[c])
                    for i, z in enumerate(pts):
                        assert int(got[i, c]) == mont(horner(cc, (canon(z),))[0]), (c, i)


def test_point_count_and_field_membership_are_checked(oracle, backend, tabs):
    from certificate_stark_amd import CstarkError
    co, d_co, _ = tabs(6)[0]
    for npts in (0, 17):
        with pytest.raises(CstarkError) as e:
            backend.evaluate_polys_at(d_co, [mont(3)] * npts)
        assert e.value.code == -1           # CSTARK_ERR_INVALID_ARG
    for m in (2, 3):
        for bad in ([P] + [0] * (m - 1), [0] * (m - 1) + [P], [1] * (m - 1) + [2**64 - 1]):
            with pytest.raises(CstarkError) as e:
                backend.evaluate_polys_at_ext(d_co, bad)
            assert e.value.code == -1
    with pytest.raises(CstarkError) as e:
        backend.evaluate_polys_at_ext(d_co, [1, 2, 3, 4])     # no such extension
    assert e.value.code == -1


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("m", [2, 3])
def test_point_evaluation_ext(oracle, backend, tabs, m, log_n):
    """cstark_evaluate_polys_at_ext at random, embedded, degenerate and saturated points against the oracle; Python-integer Horner for
    every point at n <= 512, and at 2^15 for the saturated column at the two points that drive the lazy sums highest"""
    pts = ext_points(oracle, log_n, m)
    for co, d_co, first in tabs(log_n):
        saturated = co.shape[0] == 1 and first in (SATURATED, GAPPED)
        for i, z in enumerate(pts):
            got = backend.evaluate_polys_at_ext(d_co, z)
            assert got.shape == (co.shape[0], m)
            assert (got == oracle.evaluate_polys_at_ext(co, z)).all(), (co.shape, i)
            if log_n <= 9 or (log_n == 15 and saturated and (z[0] == oracle.root_of_unity(8) or z == [P - 1] * m)):
                for c in range(co.shape[0]):
                    assert [int(v) for v in got[c]] == words(horner(canon_list(oracle, co[c]), tup(z))), (c, i)


@pytest.mark.parametrize("log_n", SIZES)
def test_known_answers_on_the_trace_domain(oracle, backend, log_n):
    """the interpolant of ev at w_n^j is ev[j] and at 0 its constant coefficient -- in the extensions as embedded elements"""
    n = 1 << log_n
    ev = oracle.random_elements(3 * n, 31 + log_n).reshape(3, n)
    co = oracle.interpolate_columns(ev)
    d_co = backend.from_numpy_u64(co)
    js = [0, 1, n // 2 + 1, n - 1]
    wn = np.array([oracle.root_of_unity(log_n)], np.uint64)
    pts = [int(oracle.fp_pow(wn, j)[0]) for j in js] + [0]
    want = [ev[:, j] for j in js] + [co[:, 0]]
    got = backend.evaluate_polys_at(d_co, pts)
    for i in range(len(pts)):
        assert (got[i] == want[i]).all(), i
    for m in (2, 3):
        for i, z in enumerate(pts):
            g = backend.evaluate_polys_at_ext(d_co, [z] + [0] * (m - 1))
            assert (g[:, 0] == want[i]).all() and not g[:, 1:].any(), (m, i)


def lazy_sum_peak(values, factor, window):
    """the largest value the 128-bit accumulator of k_poly_eval_ext_partial takes for one lane: products value * factor, and after every
    `window` of them one conditional subtraction of 2p * 2^64 (acc_fold)"""
    acc = peak = 0
    for k, v in enumerate(values):
        acc += v * factor
        peak = max(peak, acc)
        if k % window == window - 1 and (acc >> 64) >= 2 * P:
            acc -= (2 * P) << 64
    return peak


def test_lazy_sum_model_of_the_extension_evaluation():
    """At a point whose 256th power is 1 (the embedded 256th root of unity of the tests above) the table of powers holds the word
    mont(1) in component 0, and a lane of a full segment adds 64 products coefficient * mont(1).

    The all-(p - 1) column: with the kernel's window of 7 products between folds the accumulator peaks at 0.867 of 2^128 -- no wrap.
    The same input would not wrap a window of 8 (0.951).  It would not wrap a window of 9 either (0.676): nine such products exceed
    2p * 2^64, so every fold of a window of 9 subtracts and the sum never climbs.  A longer window wraps when a window that ends just
    below the fold threshold is followed by a full one, which is what the gapped column presents: p - 1 everywhere but 0 in the ninth
    coefficient of every lane.  With a window of 9 it reaches 1.128 of 2^128 (eight products, no fold, a full window on top); with the
    kernel's 7 it stays at 0.903 and with 8 at 0.892.  The bit-exact comparisons of both columns at 2^14 and above pin the window."""
    one, lane = mont(1), 16384 // 256
    saturated, gapped = [P - 1] * lane, [P - 1] * 8 + [0] + [P - 1] * (lane - 9)
    share = {(name, w): lazy_sum_peak(col, one, w) / 2**128 for name, col in (("saturated", saturated), ("gapped", gapped)) for w in (7, 8, 9)}
    print("lazy sum peaks as shares of 2^128:", {k: round(v, 4) for k, v in share.items()})
    assert 0.86 <= share["saturated", 7] < 1
    assert share["saturated", 8] < 1 and share["saturated", 9] < 1
    assert 0.86 <= share["gapped", 7] < 1 and share["gapped", 8] < 1
    assert share["gapped", 9] >= 1
    # no input can wrap the window of 7: a folded accumulator below 2p * 2^64 plus seven products of reduced operands
    assert ((2 * P) << 64) + 7 * (P - 1) ** 2 < 2**128


# ---- B. DEEP composition on synthetic tables ------------------------------------------------------------------------------------------
# (width, n_comp, log_n, log_blowup): every remainder of the fold-every-4 loops, the AIRs' own widths, columns shorter than a workgroup
DEEP_SHAPES = [(5, 2, 6, 1), (94, 8, 6, 2), (1, 1, 8, 3), (2, 4, 10, 4), (3, 8, 8, 2), (4, 1, 10, 1), (14, 2, 10, 3), (56, 4, 8, 4), (65, 8, 6, 3),
               (94, 8, 10, 3)]
N_INPUT_KINDS = 4


def deep_inputs(oracle, kind, m, width, nb, log_n, log_b, seed=0):
    """0: uniformly random.  1-3: tables whose cells are drawn from the extreme words, with coefficients all p - 1 / all (p+1)/2 / all
    zero but one, frames of zeros (v - ood = p - 1 for v = p - 1) / extreme words / p - 1, and deg_a, deg_b in 0, p - 1, mont(1)"""
    n, b = 1 << log_n, 1 << log_b
    rng = np.random.default_rng(1000 * kind + 100 * m + width + nb + log_n + log_b + seed)
    ext = np.array(EXT, np.uint64)

    def rnd(*shape):
        return oracle.to_mont(rng.integers(0, P, size=int(np.prod(shape)), dtype=np.uint64)).reshape(shape)

    def full(v, *shape):
        return np.full(shape, v, np.uint64)

    d = {}
    if kind == 0:
        d["trace_lde"], d["comp_lde"] = rnd(b, width, n), rnd(b, m * nb, n)
        d["ood_t"], d["ood_c"] = rnd(2, width, m), rnd(nb, m)
        d["al"], d["be"], d["de"] = rnd(width, m), rnd(width, m), rnd(nb, m)
        d["da"], d["db"] = rnd(m), rnd(m)
        return d
    d["trace_lde"], d["comp_lde"] = ext[rng.integers(0, 5, size=(b, width, n))], ext[rng.integers(0, 5, size=(b, m * nb, n))]
    if kind == 1:
        d["al"], d["be"], d["de"] = full(P - 1, width, m), full(P - 1, width, m), full(P - 1, nb, m)
        d["ood_t"], d["ood_c"] = full(0, 2, width, m), full(0, nb, m)
        d["da"], d["db"] = full(0, m), full(P - 1, m)
    elif kind == 2:
        d["al"], d["be"], d["de"] = full(EXT[3], width, m), full(EXT[3], width, m), full(EXT[3], nb, m)
        d["ood_t"], d["ood_c"] = ext[rng.integers(0, 5, size=(2, width, m))], ext[rng.integers(0, 5, size=(nb, m))]
        d["da"], d["db"] = full(P - 1, m), full(mont(1), m)
    else:
        d["al"], d["be"], d["de"] = full(0, width, m), full(0, width, m), full(0, nb, m)
        d["al"][-1], d["be"][0], d["de"][-1] = P - 1, P - 1, P - 1
        d["ood_t"], d["ood_c"] = full(P - 1, 2, width, m), full(P - 1, nb, m)
        d["da"], d["db"] = full(mont(1), m), full(0, m)
    return d


def lde_point(log_n, log_b, k, j):
    V = _V()
    return V.GEN * pow(V.root_of_unity(log_n + log_b), k, P) * pow(V.root_of_unity(log_n), j, P) % P


def deep_points(oracle, m, log_n, log_b):
    """memory-form m-tuples.  m = 1: random, the word p - 1, 0, 1.  m > 1: random, an embedded base element, the adjoined root, every
    component p - 1, and a z whose first component is a point x of the LDE domain while a higher one is not zero (x - z_0 = 0)"""
    r = [int(v) for v in oracle.random_elements(m + 1, 555 + m + log_n + log_b)]
    if m == 1:
        return [[r[0]], [P - 1], [0], [mont(1)]]
    x = mont(lde_point(log_n, log_b, 1, 5))
    return [r[:m], [r[m]] + [0] * (m - 1), [0, mont(1)] + [0] * (m - 2), [P - 1] * m, [x] + [0] * (m - 2) + [P - 1]]


def assert_outside_domain(z, nb, log_n, log_b):
    """No test feeds a z for which z, z w or z^nb is a point of the LDE domain g <w_(b n)>: there a divisor x - z is zero, the kernels'
    shared inversion (one inverse of the product of the three norms) then returns 0 for all three quotients while the oracle inverts each
    divisor on its own and zeroes only one -- they differ there by design, and a proof never draws such a point."""
    V = _V()
    zt, N = tup(z), 1 << (log_n + log_b)
    for e in (zt, x_scale(zt, V.root_of_unity(log_n)), x_pow(zt, nb)):
        if not any(e[1:]):
            assert pow(e[0], N, P) != pow(V.GEN, N, P), "the point lies in the LDE domain"


def deep_reference_ints(oracle, d, m, z, log_n, log_b, k0=0, nk=None):
    """the DEEP composition formula (csrc/deep.hip header) in Python integers on the cosets [k0, k0 + nk): [m][nk][n] words"""
    V = _V()
    n, b = 1 << log_n, 1 << log_b
    nk = b - k0 if nk is None else nk
    width, nb = d["trace_lde"].shape[1], d["comp_lde"].shape[1] // m
    T = np.array(canon_list(oracle, d["trace_lde"]), dtype=object).reshape(b, width, n)
    H = np.array(canon_list(oracle, d["comp_lde"]), dtype=object).reshape(b, m * nb, n)
    tt = lambda a: [tup(row) for row in np.asarray(a, np.uint64).reshape(-1, m)]
    ood_t, ood_c, al, be, de = tt(d["ood_t"]), tt(d["ood_c"]), tt(d["al"]), tt(d["be"]), tt(d["de"])
    da, db = tup(d["da"]), tup(d["db"])
    zt = tup(z)
    zw, zb = x_scale(zt, V.root_of_unity(log_n)), x_pow(zt, nb)
    out = np.zeros((m, nk, n), np.uint64)
    for k in range(k0, k0 + nk):
        for j in range(n):
            x = lde_point(log_n, log_b, k, j)
            xe = x_base(x, m)
            s1 = s2 = s3 = (0,) * m
            for c in range(width):
                t = x_base(int(T[k, c, j]), m)
                s1 = x_add(s1, x_mul(al[c], x_sub(t, ood_t[c])))
                s2 = x_add(s2, x_mul(be[c], x_sub(t, ood_t[width + c])))
            for i in range(nb):
                h = tuple(int(H[k, m * i + q, j]) for q in range(m))
                s3 = x_add(s3, x_mul(de[i], x_sub(h, ood_c[i])))
            acc = x_add(x_add(x_mul(s1, x_inv(x_sub(xe, zt))), x_mul(s2, x_inv(x_sub(xe, zw)))), x_mul(s3, x_inv(x_sub(xe, zb))))
            acc = x_mul(acc, x_add(da, x_scale(db, x)))
            out[:, k - k0, j] = words(acc)
    return out


def deep_oracle(oracle, d, m, z, log_b):
    """[m][b][n] from the oracle (the base-field function returns [b][n])"""
    if m == 1:
        return oracle.deep_composition(d["trace_lde"], d["comp_lde"], z[0], d["ood_t"], d["ood_c"], d["al"], d["be"], d["de"], int(d["da"][0]),
                                       int(d["db"][0]), log_b)[None]
    return oracle.deep_composition_ext(d["trace_lde"], d["comp_lde"], z, d["ood_t"], d["ood_c"], d["al"], d["be"], d["de"], d["da"], d["db"], log_b)


def deep_gpu(backend, d, dev, m, z, log_b, k0=0, nk=None):
    from certificate_stark_amd.backend import to_numpy_u64
    d_lde, d_clde = dev
    if m == 1:
        if nk is not None:
            d_lde, d_clde = d_lde[k0:k0 + nk].contiguous(), d_clde[k0:k0 + nk].contiguous()
        return to_numpy_u64(backend.deep_composition(d_lde, d_clde, z[0], d["ood_t"], d["ood_c"], d["al"], d["be"], d["de"], int(d["da"][0]),
                                                     int(d["db"][0]), log_b, k0=k0))[None]
    return to_numpy_u64(backend.deep_composition_ext(d_lde, d_clde, z, d["ood_t"], d["ood_c"], d["al"], d["be"], d["de"], d["da"], d["db"], log_b))


@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=lambda s: "w%d_c%d_n%d_b%d" % s)
@pytest.mark.parametrize("m", [1, 2, 3])
def test_deep_composition_matches_the_oracle(oracle, backend, m, shape):
    width, nb, log_n, log_b = shape
    b = 1 << log_b
    assert mont(_V().GEN) == oracle.generator()
    pts = deep_points(oracle, m, log_n, log_b)
    for kind in range(N_INPUT_KINDS):
        d = deep_inputs(oracle, kind, m, width, nb, log_n, log_b)
        dev = (backend.from_numpy_u64(d["trace_lde"]), backend.from_numpy_u64(d["comp_lde"]))
        for i, z in enumerate(pts):
            assert_outside_domain(z, nb, log_n, log_b)
            ref = deep_oracle(oracle, d, m, z, log_b)
            got = deep_gpu(backend, d, dev, m, z, log_b)
            assert got.shape == ref.shape == (m, b, 1 << log_n)
            assert (got == ref).all(), (kind, i)
            if m == 1:   # coset subsets, the last coset alone among them
                for k0, nk in [(b - 1, 1)] + ([(1, 2)] if b >= 4 else []):
                    assert (deep_gpu(backend, d, dev, m, z, log_b, k0, nk) == ref[:, k0:k0 + nk]).all(), (kind, i, k0)


@pytest.mark.parametrize("shape", DEEP_SHAPES[:2], ids=lambda s: "w%d_c%d_n%d_b%d" % s)
@pytest.mark.parametrize("m", [1, 2, 3])
def test_deep_composition_matches_python_integers(oracle, backend, m, shape):
    """n = 64, blowup 2 (width 5, 2 composition columns) and blowup 4 (width 94, 8 columns): every point kind, the input kinds in turn"""
    width, nb, log_n, log_b = shape
    for i, z in enumerate(deep_points(oracle, m, log_n, log_b)):
        assert_outside_domain(z, nb, log_n, log_b)
        d = deep_inputs(oracle, i % N_INPUT_KINDS, m, width, nb, log_n, log_b, seed=7)
        dev = (backend.from_numpy_u64(d["trace_lde"]), backend.from_numpy_u64(d["comp_lde"]))
        ints = deep_reference_ints(oracle, d, m, z, log_n, log_b)
        assert (deep_oracle(oracle, d, m, z, log_b) == ints).all(), ("oracle", i)
        assert (deep_gpu(backend, d, dev, m, z, log_b) == ints).all(), ("kernel", i)


@pytest.fixture(scope="module")
def real_stage(oracle):
    """a real trace (2 transfers), its extension, and real composition columns for three coefficient sets"""
    w = oracle.TxWitness.generate(2, 3, seed=606)
    trace = oracle.tx_build_trace(w)
    log_b = 3
    co = oracle.interpolate_columns(trace)
    lde = oracle.lde_columns(co, log_b)
    pub = np.concatenate([w.initial_roots[0][:2], w.final_root[:2]])
    cols = [oracle.composition_columns(oracle.tx_evaluate_constraints(lde, oracle.make_coeffs(3 + q), pub, w.depth, log_b)) for q in range(3)]
    return co, lde, cols


def recombine(raw, m, nb):
    """H_i = sum_q root^q H_(i,q): raw [m nb][m] words (component column m i + q at the point) -> [nb][m] words"""
    out = np.zeros((nb, m), np.uint64)
    root = (0, 1) + (0,) * (m - 2)
    for i in range(nb):
        h, rq = (0,) * m, x_base(1, m)
        for q in range(m):
            h = x_add(h, x_mul(rq, tup(raw[m * i + q])))
            rq = x_mul(rq, root)
        out[i] = words(h)
    return out


@pytest.mark.parametrize("m", [1, 2, 3])
def test_deep_composition_of_a_real_trace_is_of_low_degree(oracle, backend, real_stage, m):
    """oracle-free: with the true frame (the point evaluations of section A) every component of the DEEP composition of a real trace and
    real composition columns interpolates to a polynomial of degree below n"""
    co, lde, cols = real_stage
    n = co.shape[1]
    log_n, log_b, nb = n.bit_length() - 1, 3, 8
    ccols = np.stack([cols[q][i] for i in range(nb) for q in range(m)])             # column m i + q = component q of composition column i
    comp_lde = oracle.lde_columns(ccols, log_b)
    z = [int(v) for v in oracle.random_elements(m, 808 + m)]
    assert_outside_domain(z, nb, log_n, log_b)
    zt = tup(z)
    zw, zb = words(x_scale(zt, _V().root_of_unity(log_n))), words(x_pow(zt, nb))
    d_co, d_cc = backend.from_numpy_u64(co), backend.from_numpy_u64(ccols)
    if m == 1:
        ood_t = backend.evaluate_polys_at(d_co, [z[0], zw[0]])
        ood_c = backend.evaluate_polys_at(d_cc, zb)[0]
    else:
        ood_t = np.stack([backend.evaluate_polys_at_ext(d_co, z), backend.evaluate_polys_at_ext(d_co, zw)])
        ood_c = recombine(backend.evaluate_polys_at_ext(d_cc, zb), m, nb)
    d = {"trace_lde": lde, "comp_lde": comp_lde, "ood_t": ood_t, "ood_c": ood_c, "da": oracle.random_elements(m, 5), "db": oracle.random_elements(m, 6)}
    d["al"], d["be"], d["de"] = (oracle.random_elements(k * m, s).reshape(k, m) for k, s in ((94, 1), (94, 2), (nb, 3)))
    got = deep_gpu(backend, d, (backend.from_numpy_u64(lde), backend.from_numpy_u64(comp_lde)), m, z, log_b)
    assert got.any()
    for q in range(m):
        nat = np.ascontiguousarray(got[q].T).ravel()
        assert not oracle.ntt(nat, inverse=True)[n:].any(), q


# ---- C. the device-resident forms -----------------------------------------------------------------------------------------------------
def ood_deep_dev(backend, m, pts, d_co, d_cc, dev, coef, deg, shifts, nk, log_n, log_b, ood_in=None):
    """cstark_debug_ood_deep_dev with every operand placed in device memory -> (frame [2 width + nb][m], sums [m][nk][n])"""
    from certificate_stark_amd import _lib
    from certificate_stark_amd.backend import to_numpy_u64
    width, nb = d_co.shape[0], d_cc.shape[0] // m
    up = lambda a: backend.from_numpy_u64(np.ascontiguousarray(a, np.uint64).reshape(-1))
    d_pts, d_coef, d_deg, d_shifts = up(pts), up(coef), up(deg), up(shifts)
    d_in = up(ood_in) if ood_in is not None else None
    d_scal = backend.from_numpy_u64(np.full(8 * m, 0x5555555555555555, np.uint64))
    # the sums get room for all 2^log_b cosets behind a sentinel: an output stride other than nk shows as a mismatch, not as a stray write
    n, b = 1 << log_n, 1 << log_b
    sentinel = 0x7777777777777777
    d_frame, d_sums = backend.empty_u64((2 * width + nb) * m), backend.from_numpy_u64(np.full(m * b * n, sentinel, np.uint64))
    p = backend._ptr
    rc = _lib.load_debug().cstark_debug_ood_deep_dev(backend.ctx, C.c_uint32(m), p(d_pts), p(d_co), C.c_uint32(width), p(d_cc), C.c_uint32(nb), p(dev[0]),
                                                     p(dev[1]), p(d_coef), p(d_deg), p(d_shifts), p(d_in) if d_in is not None else None, p(d_scal),
                                                     C.c_uint32(nk), C.c_uint32(log_n), C.c_uint32(log_b), p(d_frame), p(d_sums))
    assert rc == 0
    sums = to_numpy_u64(d_sums)
    assert (sums[m * nk * n:] == sentinel).all(), "the quotient sums were written past [m][nk][n]"
    return to_numpy_u64(d_frame).reshape(-1, m), sums[:m * nk * n].reshape(m, nk, n)


# 2 width + n_comp = 12, 196 and 264: one pass and two passes of the stride loop of k_deep_ext_consts
@pytest.mark.parametrize("width,nb", [(5, 2), (94, 8), (130, 4)])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_device_resident_frame_and_quotient_sums(oracle, backend, m, width, nb):
    """what prove.hip runs when the channel is on the device: the frame equals the host-argument evaluations (and, for m > 1, the
    recombination in Python tuples); the quotient sums on the first nk cosets equal the host-argument composition and the oracle"""
    log_n, log_b = 10, 3
    n, b = 1 << log_n, 1 << log_b
    co = oracle.random_elements(width * n, 61 + m).reshape(width, n)
    cc = oracle.random_elements(m * nb * n, 62 + m).reshape(m * nb, n)
    d_co, d_cc = backend.from_numpy_u64(co), backend.from_numpy_u64(cc)
    shifts = [mont(lde_point(log_n, log_b, k, 0)) for k in range(b)]
    for i, z in enumerate(deep_points(oracle, m, log_n, log_b)[:4]):
        assert_outside_domain(z, nb, log_n, log_b)
        zt = tup(z)
        zw, zb = words(x_scale(zt, _V().root_of_unity(log_n))), words(x_pow(zt, nb))
        if m == 1:
            ood_t = backend.evaluate_polys_at(d_co, [z[0], zw[0]]).reshape(2, width, 1)
            ood_c = backend.evaluate_polys_at(d_cc, zb).reshape(nb, 1)
            assert (ood_t[:, :, 0] == oracle.evaluate_polys_at(co, [z[0], zw[0]])).all()
        else:
            ood_t = np.stack([backend.evaluate_polys_at_ext(d_co, z), backend.evaluate_polys_at_ext(d_co, zw)])
            ood_c = recombine(backend.evaluate_polys_at_ext(d_cc, zb), m, nb)
            assert (ood_t[0] == oracle.evaluate_polys_at_ext(co, z)).all()
        frame = np.concatenate([ood_t.reshape(-1, m), ood_c])
        saturated = np.full_like(frame, P - 1)
        # (inputs, frame the DEEP stage reads): the computed frame with random and with extreme tables; an all-(p - 1) frame with all-(p - 1) coefficients
        for kind, given in ((0, None), (2, None), (1, saturated)):
            d = deep_inputs(oracle, kind, m, width, nb, log_n, log_b, seed=i)
            f = frame if given is None else given
            d["ood_t"], d["ood_c"] = f[:2 * width].reshape(2, width, m), f[2 * width:]
            dev = (backend.from_numpy_u64(d["trace_lde"]), backend.from_numpy_u64(d["comp_lde"]))
            ref = deep_oracle(oracle, d, m, z, log_b)
            assert (deep_gpu(backend, d, dev, m, z, log_b) == ref).all(), (i, kind)
            coef, deg = np.concatenate([d["al"], d["be"], d["de"]]), np.concatenate([d["da"], d["db"]])
            for nk in (1, 3, b):
                got_frame, sums = ood_deep_dev(backend, m, z + zw + zb, d_co, d_cc, dev, coef, deg, shifts, nk, log_n, log_b, given)
                assert (got_frame == frame).all(), (i, kind, nk)
                assert (sums == ref[:, :nk]).all(), (i, kind, nk)
