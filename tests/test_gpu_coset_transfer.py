"""The kernels that carry polynomials between cosets as coefficient vectors, one at a time through include/cstark_debug_coset.h:
k_coset_even_to_odd (with its coset window), k_coset_even_to_odd_merged and k_coset_combine of csrc/ntt.hip, k_final_hi,
k_final_hi_merge and k_shard_combine of csrc/constraints.hip.  The references (tests/coset_cases.py, themselves checked without a GPU
by test_coset_reference_cpu.py) state what the vectors mean and compute it with the oracle's transforms.  Exact field arithmetic: every
comparison is bit for bit.  Every output buffer starts as 0xA5 bytes, carries n spare words at its end and is compared whole.

On k_coset_combine's fold at k == 6: it can never fire.  Seven products of reduced elements are below 7 p^2 = 1.79 p 2^64 < 2 p 2^64,
the threshold of acc_fold; and all eight are below 8 p^2 = 2.05 p 2^64 < 2^128, which the fold at the end brings under 2 p 2^64 as
acc_reduce requires.  No input tells the kernel with that fold from the kernel without it; the all-(p - 1) and alternating inputs below
drive the accumulator as high as it goes."""
import numpy as np
import pytest

import coset_cases as K
from coset_cases import G, HIP_INVALID_VALUE, HIP_SUCCESS, P
from test_gpu_split_merge import assert_adjustments_exercise_the_carry, group_adjustment

pytestmark = pytest.mark.gpu
SIZES = [256, 1024]   # one workgroup per table and the smallest the unguarded launchers accept | several workgroups, the stage's smallest


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def dev(backend):
    return K.CosetDev(backend)


@pytest.fixture(scope="module")
def ref(oracle):
    return K.Ref(oracle)


def log2(n):
    return n.bit_length() - 1


def mixed_tables(ref, rng, tables, n):
    """[tables][4][n] interpolants: table t takes pattern t mod 7 of random | all p - 1 | alternating | the impulses a_t = 1 at
    t = 0, n - 1, n, 4n - 1 (as the interpolants of that polynomial)"""
    fam = K.input_families((4, n), rng)
    out = np.empty((tables, 4, n), np.uint64)
    for t in range(tables):
        kind = t % 7
        if kind == 0:
            out[t] = rng.integers(0, P, size=(4, n), dtype=np.uint64)
        elif kind < 3:
            out[t] = fam[("all p-1", "alternating")[kind - 1]]
        else:
            out[t] = ref.even_interpolants(K.impulse(ref, 4 * n, (0, n - 1, n, 4 * n - 1)[kind - 3]))
    return out


def run_plain(dev, d_in_np, n, kc0=0, nkc=4):
    tables = d_in_np.shape[0]
    d_out = dev.filled(4 * tables * n + n)
    assert dev.even_to_odd(dev.u64(d_in_np), d_out, log2(n), tables, kc0, nkc) == HIP_SUCCESS
    return dev.words_of(d_out)


# ---- the plain extension ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_plain_extension_on_every_input_family(dev, ref, n):
    rng = np.random.default_rng(n)
    d_in = mixed_tables(ref, rng, 7, n)
    got = run_plain(dev, d_in, n)
    want = K.expected_buffer(got.size, ref.even_to_odd(d_in))
    where = np.argwhere((got != want)[:28 * n].reshape(4, 7, n))[:, :2].tolist()
    assert (got == want).all(), "(coset, table) that differ: %s" % sorted(set(map(tuple, where)))
    # an impulse a_t = 1, t = q + n i, must come out as W8^(k' i) at q and nothing else
    w8 = pow(ref.root(log2(n) + 3), n, P)
    for table, t in ((3, 0), (4, n - 1), (5, n), (6, 4 * n - 1)):
        i, q = divmod(t, n)
        for kc in range(4):
            vec = ref.ints(got[(kc * 7 + table) * n:(kc * 7 + table + 1) * n])
            assert vec[q] == pow(w8, (2 * kc + 1) * i, P) and sum(1 for v in vec if v) == 1, (t, kc)


@pytest.mark.parametrize("tables", [1, 4, 13])
@pytest.mark.parametrize("n", SIZES)
def test_plain_extension_windows(dev, ref, n, tables):
    """All ten windows [kc0, kc0 + nkc) of the four even cosets.  The absent cosets hold words that are no field elements: they must
    not be read.  The shares of a partition add up to the whole."""
    rng = np.random.default_rng(100 * tables + n)
    d_in = mixed_tables(ref, rng, tables, n)
    got = {}
    for kc0 in range(4):
        for nkc in range(1, 5 - kc0):
            junk = np.full_like(d_in, K.NOT_A_FIELD_ELEMENT)
            junk[:, kc0:kc0 + nkc] = d_in[:, kc0:kc0 + nkc]
            got[(kc0, nkc)] = run_plain(dev, junk, n, kc0, nkc)
            want = K.expected_buffer(got[(kc0, nkc)].size, ref.even_to_odd(d_in, kc0, nkc))
            assert (got[(kc0, nkc)] == want).all(), "window (%d, %d)" % (kc0, nkc)
    live = 4 * tables * n
    whole = got[(0, 4)][:live]
    assert (K.add_mod_p(ref, [got[(0, 2)][:live], got[(2, 2)][:live]]) == whole).all()
    assert (K.add_mod_p(ref, [got[(kc, 1)][:live] for kc in range(4)]) == whole).all()


def test_plain_extension_refusals(dev):
    n = 256
    d_in, d_out = dev.u64(np.zeros(4 * n, np.uint64)), dev.filled(5 * n)
    bad = [dict(nkc=0), dict(kc0=1, nkc=4), dict(kc0=4, nkc=1), dict(kc0=5, nkc=0xFFFFFFFF), dict(tables=0), dict(log_n=5), dict(log_n=22),
           dict(tables=2), dict(out_words=4 * n - 1), dict(in_words=4 * n - 1)]
    for kw in bad:
        a = dict(log_n=8, tables=1, kc0=0, nkc=4, in_words=None, out_words=None)
        a.update(kw)
        assert dev.even_to_odd(d_in, d_out, a["log_n"], a["tables"], a["kc0"], a["nkc"], a["in_words"], a["out_words"]) == HIP_INVALID_VALUE, kw
    assert (dev.words_of(d_out) == K.FILL_WORD).all()
    assert dev.even_to_odd(d_in, d_out, 8, 1) == HIP_SUCCESS


# ---- the merged extension ------------------------------------------------------------------------------------------------------------------

def run_merged(dev, ref, d_in, n, families, tables_per_set, raw_family, with_raw=True, base=G, k0=1):
    """d_in [sets][tables_per_set][4][n] -> (out words, raw words or None, terms)"""
    sets = d_in.shape[0]
    d_out = dev.filled(4 * sets * len(families) * n + n)
    raw_terms = len(families[raw_family]) if raw_family >= 0 else 1
    d_raw = dev.filled(sets * raw_terms * n + n) if with_raw else None
    desc = dev.merge_desc(families, tables_per_set, raw_family, ref.mont([base])[0], k0)
    rc, terms = dev.even_to_odd_merged(dev.u64(d_in), d_out, d_raw, log2(n), sets, desc)
    assert rc == HIP_SUCCESS
    return dev.words_of(d_out), dev.words_of(d_raw) if with_raw else None, terms


def merged_expectation(ref, d_in, families, raw_family):
    """out [4][sets][families][n], raw [sets][terms][n] (or None)"""
    per_set = [ref.merged(d_in[s], families, raw_family) for s in range(d_in.shape[0])]
    return np.stack([o for o, _ in per_set], axis=1), (np.stack([r for _, r in per_set]) if raw_family >= 0 else None)


def assert_terms(ref, terms, families, n, base=G, k0=1):
    for f, fam in enumerate(families):
        for t, (table, e) in enumerate(fam):
            c, tab, r = terms[f][t]
            want_c, want_r = ref.merge_constants(e, n, base, k0)
            assert (tab, r) == (table, want_r), (f, t)
            assert [ref.ints(row) for row in c] == want_c, "family %d term %d (e = %d): constants" % (f, t, e)


def assert_merged(ref, got_out, got_raw, d_in, families, raw_family, what=""):
    want_out, want_raw = merged_expectation(ref, d_in, families, raw_family)
    want = K.expected_buffer(got_out.size, want_out)
    if not (got_out == want).all():
        where = np.argwhere((got_out != want)[:want_out.size].reshape(want_out.shape))
        raise AssertionError("%s: (coset, set, family) that differ: %s; words past the shape touched: %s"
                             % (what, sorted(set(map(tuple, where[:, :3].tolist()))), bool((got_out != want)[want_out.size:].any())))
    if got_raw is not None:
        want = K.expected_buffer(got_raw.size, want_raw if want_raw is not None else np.zeros(0, np.uint64))
        assert (got_raw == want).all(), "%s: the raw output differs" % what


PRODUCTION_FIRST, PRODUCTION_TERMS = (0, 4, 7, 9, 11), (4, 3, 2, 2, 2)   # TransactionAir's five flag families over its 13 split tables


def production_families(n):
    adj = [group_adjustment(g, n) for g in range(3)]
    return [[(first + t, adj[t - 1] if t else 0) for t in range(count)] for first, count in zip(PRODUCTION_FIRST, PRODUCTION_TERMS)]


@pytest.mark.parametrize("sets", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_merged_extension_in_the_production_shape(dev, ref, n, sets):
    assert_adjustments_exercise_the_carry(n)
    families = production_families(n)
    rng = np.random.default_rng(10 * n + sets)
    d_in = mixed_tables(ref, rng, sets * 13, n).reshape(sets, 13, 4, n)
    out, raw, terms = run_merged(dev, ref, d_in, n, families, 13, raw_family=4)
    assert_terms(ref, terms, families, n)
    assert_merged(ref, out, raw, d_in, families, 4, "production shape")
    # the raw output as the stage uses it: transformed as it stands, the table on LDE coset 1
    for s in range(sets):
        for t, (table, _) in enumerate(families[4]):
            vec = raw[(s * 2 + t) * n:(s * 2 + t + 1) * n]
            assert (ref.O.ntt(vec) == ref.odd_values(ref.coefficients(d_in[s, table]))[0]).all()


def steered_exponents(n):
    return [(0, 1, n - 1, n), (8 * n, 8 * n + 1, 15 * n + (n - 1), 7 * n), (2**40 + 3, 3 * n, 5 * n + 1, 9 * n - 1)]


def rotation_impulses(ref, n, r):
    """[4][n] interpolants with a single 1 each: coset slot i at the i-th of q = 0, r - 1, r, n - 1 (mod n).  Output index q' reads input
    (q' - r) mod n, so the 1 at 0 lands on q' = r, the first index that did not wrap, and the 1 at n - 1 on q' = r - 1, the last that did."""
    out = np.zeros((4, n), np.uint64)
    for i, q in enumerate((0, (r - 1) % n, r, n - 1)):
        out[i, q] = ref.mont([1])[0]
    return out


@pytest.mark.parametrize("run", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_merged_extension_one_family_of_four_terms(dev, ref, n, run):
    exps = steered_exponents(n)[run]
    families = [[(t, e) for t, e in enumerate(exps)]]
    rng = np.random.default_rng(n + run)
    random = rng.integers(0, P, size=(1, 4, 4, n), dtype=np.uint64)
    steered = np.stack([rotation_impulses(ref, n, e % n) for e in exps])[None]
    for what, d_in in (("random", random), ("impulses", steered)):
        out, raw, terms = run_merged(dev, ref, d_in, n, families, 4, raw_family=0)
        assert_terms(ref, terms, families, n)
        assert_merged(ref, out, raw, d_in, families, 0, "%s, exponents %s" % (what, exps))
    # one term alone on the impulses: the 1 the rotation carries to q' = r - 1 wrapped, the one it carries to q' = r did not
    for t, e in enumerate(exps):
        fam = [[(t, e)]]
        out, _, _ = run_merged(dev, ref, steered, n, fam, 4, raw_family=-1)
        assert_merged(ref, out, None, steered, fam, -1, "term %d alone" % t)


@pytest.mark.parametrize("raw_family", [-1, 0, 4])
@pytest.mark.parametrize("n", SIZES)
def test_merged_extension_five_single_term_families(dev, ref, n, raw_family):
    exps = (n - 1, 0, 8 * n + 1, group_adjustment(0, n), 3 * n)
    families = [[(4 - f, e)] for f, e in enumerate(exps)]   # the tables in descending order
    rng = np.random.default_rng(5 * n + raw_family)
    d_in = mixed_tables(ref, rng, 10, n).reshape(2, 5, 4, n)
    out, raw, terms = run_merged(dev, ref, d_in, n, families, 5, raw_family)
    assert_terms(ref, terms, families, n)
    assert_merged(ref, out, raw, d_in, families, raw_family, "raw_family %d" % raw_family)   # raw_family -1: d_raw stays untouched
    # without d_raw the same outputs, whatever raw_family says
    out2, _, _ = run_merged(dev, ref, d_in, n, families, 5, raw_family, with_raw=False)
    assert (out2 == out).all()


@pytest.mark.parametrize("n", SIZES)
def test_merge_constants_of_the_high_part_s_term(dev, ref, n):
    """k0 = 2 with base g w_8n, the form k_final_hi_merge consumes: the host constants as numbers (the kernel's outputs are not looked at:
    it writes the odd cosets whatever k0 says)"""
    base = G * ref.root(log2(n) + 3) % P
    exps = (group_adjustment(0, n), n - 1, 8 * n + 1, 2**40 + 3 + 5 * n)
    families = [[(0, e) for e in exps]]
    d_in = np.zeros((1, 1, 4, n), np.uint64)
    _, _, terms = run_merged(dev, ref, d_in, n, families, 1, -1, base=base, k0=2)
    assert_terms(ref, terms, families, n, base, 2)


def test_merged_extension_refusals(dev, ref):
    n = 256
    d_in, d_out, d_raw = dev.u64(np.zeros(2 * 4 * n, np.uint64)), dev.filled(4 * 5 * n + n), dev.filled(4 * n + n)
    one = ref.mont([G])[0]
    good = [[(0, 1), (1, n)]]
    six = [[(0, 0)]] * 6
    cases = [("families 0", dev.merge_desc([], 2, -1, one), 1),
             ("families 6", dev.merge_desc(six, 2, -1, one), 1),
             ("terms 0", dev.merge_desc(good, 2, -1, one, terms={0: 0}), 1),
             ("terms 5", dev.merge_desc(good, 2, -1, one, terms={0: 5}), 1),
             ("table = tables_per_set", dev.merge_desc([[(0, 1), (2, n)]], 2, -1, one), 1),
             ("raw_family = families", dev.merge_desc(good, 2, 1, one), 1),
             ("raw_family -2", dev.merge_desc(good, 2, -2, one), 1),
             ("sets 0", dev.merge_desc(good, 2, -1, one), 0),
             ("sets beyond the input", dev.merge_desc(good, 2, -1, one), 2),
             ("tables beyond the input", dev.merge_desc(good, 3, -1, one), 1),
             ("base not canonical", dev.merge_desc(good, 2, -1, P), 1),
             ("k0 3", dev.merge_desc(good, 2, -1, one, k0=3), 1)]
    for what, desc, sets in cases:
        rc, _ = dev.even_to_odd_merged(d_in, d_out, d_raw, 8, sets, desc)
        assert rc == HIP_INVALID_VALUE, what
    rc, _ = dev.even_to_odd_merged(d_in, d_out, dev.filled(n), 8, 1, dev.merge_desc(good, 2, 0, one))   # the raw output would not fit
    assert rc == HIP_INVALID_VALUE
    rc, _ = dev.even_to_odd_merged(d_in, d_out, d_raw, 5, 1, dev.merge_desc(good, 2, -1, one))
    assert rc == HIP_INVALID_VALUE
    assert (dev.words_of(d_out) == K.FILL_WORD).all() and (dev.words_of(d_raw) == K.FILL_WORD).all()
    rc, _ = dev.even_to_odd_merged(d_in, d_out, d_raw, 8, 1, dev.merge_desc(good, 2, 0, one))
    assert rc == HIP_SUCCESS


# ---- coset_combine ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tables", [1, 3])
@pytest.mark.parametrize("n", [64, 256, 1024])     # 64: a quarter-filled workgroup
@pytest.mark.parametrize("log_b", [1, 2, 3])
def test_coset_combine(dev, ref, log_b, n, tables):
    bb = 1 << log_b
    rng = np.random.default_rng(1000 * log_b + n + tables)
    a = ref.O.to_mont(rng.integers(0, P, size=(tables, bb * n), dtype=np.uint64))
    cases = [("random", np.stack([ref.combine_inputs(a[t], log_b) for t in range(tables)]), a)]
    if log_b == 3:
        fam = K.input_families((tables, bb, n), rng)
        for kind in ("all p-1", "alternating"):
            cases.append((kind, fam[kind], np.stack([ref.combine(fam[kind][t]) for t in range(tables)])))
    for what, d_b, want in cases:
        d_h = dev.filled(tables * bb * n + n)
        assert dev.coset_combine(dev.u64(d_b), d_h, log2(n), log_b, tables, words=tables * bb * n) == HIP_SUCCESS
        got = dev.words_of(d_h)
        assert (got == K.expected_buffer(got.size, want)).all(), what


def test_coset_combine_refusals(dev):
    n = 64
    d_b, d_h = dev.u64(np.zeros(16 * n, np.uint64)), dev.filled(16 * n)
    for log_n, log_b, tables, words in [(6, 0, 1, 16 * n), (6, 4, 1, 16 * n), (5, 1, 1, 16 * n), (6, 3, 0, 16 * n), (6, 3, 3, 16 * n), (6, 3, 1, 8 * n - 1),
                                        (22, 3, 1, 16 * n)]:
        assert dev.coset_combine(d_b, d_h, log_n, log_b, tables, words) == HIP_INVALID_VALUE, (log_n, log_b, tables, words)
    assert dev.coset_combine(d_b, d_b, 6, 3, 1, 16 * n) == HIP_INVALID_VALUE
    assert (dev.words_of(d_h) == K.FILL_WORD).all()


# ---- the high part of the final addition ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 11, 2, 13), (6, 11, 2, 13), (3, 8, 3, 11)])   # (rows, first, per_set, tables_per_set)
@pytest.mark.parametrize("n", SIZES)
def test_final_hi(dev, ref, n, shape):
    rows, first, per_set, tps = shape
    blocks = rows // per_set
    rng = np.random.default_rng(n + rows)
    odd_f, dir_f = K.input_families((blocks * tps, n), rng), K.input_families((rows, n), rng)
    cases = [("random", odd_f["random"], dir_f["random"]),
             ("0 - (p - 1)", np.zeros((blocks * tps, n), np.uint64), dir_f["all p-1"]),   # the subtraction wraps everywhere
             ("(p - 1) - alternating", odd_f["all p-1"], dir_f["alternating"]),
             ("alternating - random", odd_f["alternating"], dir_f["random"])]
    for what, odd, direct in cases:
        # every table of `odd` that is not a sum's table is no field element: reading a wrong one shows
        marked = np.full_like(odd, K.NOT_A_FIELD_ELEMENT)
        for r in range(rows):
            t = (r // per_set) * tps + first + r % per_set
            marked[t] = odd[t]
        d_hi = dev.filled(rows * n + n)
        assert dev.final_hi(dev.u64(marked), dev.u64(direct), d_hi, log2(n), rows, first, per_set, tps) == HIP_SUCCESS
        got = dev.words_of(d_hi)
        assert (got == K.expected_buffer(got.size, ref.final_hi(odd, direct, first, per_set, tps))).all(), what


def test_final_hi_refusals(dev):
    n = 256
    d_odd, d_direct, d_hi = dev.u64(np.zeros(13 * n, np.uint64)), dev.u64(np.zeros(2 * n, np.uint64)), dev.filled(2 * n)
    for log_n, rows, first, per_set, tps in [(7, 2, 11, 2, 13), (8, 0, 11, 2, 13), (8, 2, 11, 0, 13), (8, 3, 11, 2, 13), (8, 2, 12, 2, 13), (8, 4, 11, 2, 13),
                                             (8, 2, 0xFFFFFFFF, 2, 13), (9, 2, 11, 2, 13)]:
        assert dev.final_hi(d_odd, d_direct, d_hi, log_n, rows, first, per_set, tps) == HIP_INVALID_VALUE, (log_n, rows, first, per_set, tps)
    assert (dev.words_of(d_hi) == K.FILL_WORD).all()


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_final_hi_merge(dev, ref, n, m):
    base = G * ref.root(log2(n) + 3) % P
    base_word = ref.mont([base])[0]
    rng = np.random.default_rng(7 * n + m)
    for e in (group_adjustment(0, n), n - 1, 8 * n + 1):
        r = e % n
        imp_t = np.zeros((m, 2, n), np.uint64)
        for c in range(m):
            imp_t[c, 0, (c + 1) % n] = ref.mont([2])[0]
            for q in ((0, n - 1), ((r - 1) % n, r), (0, r))[c]:       # slot 1: the ends of the rotation, set by set
                imp_t[c, 1, q] = ref.mont([2])[0]
        cases = [("random", rng.integers(0, P, size=(m, 2, n), dtype=np.uint64), rng.integers(0, P, size=(m, 2, n), dtype=np.uint64)),
                 ("impulses", imp_t, np.zeros((m, 2, n), np.uint64)),
                 ("0 - (p - 1)", np.zeros((m, 2, n), np.uint64), np.full((m, 2, n), P - 1, np.uint64))]
        for what, tco, qco in cases:
            d_out = dev.filled(3 * m * n + n)
            rc, term = dev.final_hi_merge(dev.u64(tco), dev.u64(qco), d_out, log2(n), m, e, base_word, 2)
            assert rc == HIP_SUCCESS
            c, table, got_r = term
            assert (table, got_r) == (0, r) and [ref.ints(row) for row in c] == ref.merge_constants(e, n, base, 2)[0]
            got = dev.words_of(d_out)
            assert (got == K.expected_buffer(got.size, ref.final_hi_merge(tco, qco, e, base, 2))).all(), (what, e)


def test_final_hi_merge_refusals(dev, ref):
    n = 256
    d_t, d_q, d_out = dev.u64(np.zeros(4 * n, np.uint64)), dev.u64(np.zeros(4 * n, np.uint64)), dev.filled(6 * n)
    g = ref.mont([G])[0]
    for log_n, m, base, k0 in [(7, 1, g, 2), (8, 0, g, 2), (8, 4, g, 2), (8, 3, g, 2), (8, 2, P, 2), (8, 2, g, 0), (8, 2, g, 3), (9, 2, g, 2), (22, 1, g, 2)]:
        rc, _ = dev.final_hi_merge(d_t, d_q, d_out, log_n, m, n + 1, base, k0)
        assert rc == HIP_INVALID_VALUE, (log_n, m, base, k0)
    assert (dev.words_of(d_out) == K.FILL_WORD).all()


# ---- the sharded path's data mover -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nkc", [1, 2])
def test_shard_combine(dev, ref, nkc):
    n = 256
    world, rows = 4 // nkc, nkc + 4
    rng = np.random.default_rng(nkc)
    distinct = np.arange(world * rows * n, dtype=np.uint64).reshape(world, rows, n) * np.uint64(0x9E3779B1) + np.uint64(1)  # no two words alike
    wrapping = rng.integers(0, P, size=(world, rows, n), dtype=np.uint64)
    wrapping[:, nkc:] = P - 1                                                                    # the sums over the ranks wrap
    for what, parts in (("distinct", distinct), ("all p - 1 in the odd cosets' rows", wrapping)):
        assert (parts < P).all()
        d_out = dev.filled(8 * n + n)
        assert dev.shard_combine(dev.u64(parts), d_out, log2(n), nkc) == HIP_SUCCESS
        got = dev.words_of(d_out)
        assert (got == K.expected_buffer(got.size, ref.shard_combine(parts, nkc))).all(), what


def test_shard_combine_refusals(dev):
    n = 256
    d_parts, d_out = dev.u64(np.zeros(12 * n, np.uint64)), dev.filled(8 * n)
    for log_n, nkc in [(8, 0), (8, 3), (8, 4), (7, 2), (9, 2), (8, 1)]:      # nkc = 1 needs 20 n words of parts
        assert dev.shard_combine(d_parts, d_out, log_n, nkc) == HIP_INVALID_VALUE, (log_n, nkc)
    assert (dev.words_of(d_out) == K.FILL_WORD).all()
    assert dev.shard_combine(d_parts, d_out, 8, 2) == HIP_SUCCESS
