"""No GPU: the references that test_gpu_coset_transfer.py holds the coset-transfer kernels to (tests/coset_cases.py) are checked here
against each other -- transform form against closed form -- and against the oracle's own interpolation and extension, so that a GPU
failure there points at the kernel and not at the test."""
import numpy as np
import pytest

import coset_cases as K
from coset_cases import G, P


@pytest.fixture(scope="module")
def ref(oracle):
    return K.Ref(oracle)


def random_words(ref, rng, *shape):
    return ref.O.to_mont(rng.integers(0, P, size=int(np.prod(shape)), dtype=np.uint64)).reshape(shape)


def test_the_oracle_transform_is_the_plain_sum(ref):
    """oracle.ntt(a)[j] = sum_t a_t w_n^(j t), and inverse=True undoes it: what every reference here builds on"""
    n = 64
    rng = np.random.default_rng(1)
    a = random_words(ref, rng, n)
    ai, w = ref.ints(a), ref.root(6)
    assert ref.ints(ref.O.ntt(a)) == [sum(ai[t] * pow(w, j * t, P) for t in range(n)) % P for j in range(n)]
    assert (ref.O.ntt(ref.O.ntt(a), inverse=True) == a).all()
    assert pow(ref.root(9), 2, P) == ref.root(8) and pow(ref.root(8), 4, P) == ref.root(6)
    assert pow(ref.root(9), 64 * 8, P) == 1 and pow(ref.root(9), 64 * 4, P) == P - 1


@pytest.mark.parametrize("n", [64, 256])
def test_even_to_odd_forms_agree(ref, n):
    rng = np.random.default_rng(n)
    a = random_words(ref, rng, 4 * n)
    b = ref.even_interpolants(a)
    assert (b == ref.even_interpolants_closed(a)).all()
    assert (ref.coefficients(b) == a).all()
    out = ref.odd_vectors(a)
    assert (out == ref.odd_vectors_closed(a)).all()
    assert (ref.even_to_odd(b[None])[:, 0] == out).all()
    # the oracle's own extension: x-coefficients c_t = a_t g^-t, the 8n-point LDE domain in natural order, point 8 j + k
    c = ref.scale(a, pow(G, -1, P))
    lde = ref.O.lde_columns(c[None, :], 1)                    # [2][1][4n]: point 2 i + k of the 8n-point domain
    natural = np.ascontiguousarray(lde[:, 0, :].T).ravel()
    for kc in range(4):
        assert (ref.values_of_vector(out[kc], 2 * kc + 1) == natural[2 * kc + 1::8]).all()
        assert (ref.O.ntt(b[kc]) == natural[2 * kc::8]).all()
    # and its interpolation: the even cosets together are the 4n-point domain of y
    assert (ref.O.interpolate_columns(np.ascontiguousarray(natural[0::2])[None, :])[0] == a).all()


@pytest.mark.parametrize("n", [64, 256])
def test_windows_of_a_partition_sum_to_the_whole(ref, n):
    rng = np.random.default_rng(n + 1)
    d_in = random_words(ref, rng, 2, 4, n)
    whole = ref.even_to_odd(d_in)
    for parts in ([(0, 2), (2, 2)], [(0, 1), (1, 1), (2, 1), (3, 1)], [(0, 3), (3, 1)], [(0, 1), (1, 3)]):
        assert (K.add_mod_p(ref, [ref.even_to_odd(d_in, kc0, nkc) for kc0, nkc in parts]) == whole).all(), parts
    # what stands in an absent coset does not count
    junk = d_in.copy()
    junk[:, 0] = K.NOT_A_FIELD_ELEMENT
    junk[:, 3] = K.NOT_A_FIELD_ELEMENT
    assert (ref.even_to_odd(junk, 1, 2) == ref.even_to_odd(d_in, 1, 2)).all()
    assert ref.even_to_odd(d_in, 1, 2).any() and not (ref.even_to_odd(d_in, 1, 2) == whole).all()


def test_merged_reference_is_the_sum_of_rotated_plain_references(ref):
    """The rule test_gpu_split_merge.py restates in integers -- rotate by e mod n, the wrapped entries times y^n -- against the meaning:
    the values of sum_t x^(e_t) S_t on the odd cosets."""
    import test_gpu_split_merge as SM
    n = SM.N
    rng = np.random.default_rng(7)
    d_in = random_words(ref, rng, 4, 4, n)
    plain = ref.even_to_odd(d_in)
    for exps in SM.EXPONENT_SETS:
        families = [[(0, 0), (1, exps[0]), (2, exps[1])], [(3, exps[2])]]
        got, raw = ref.merged(d_in, families, raw_family=0)
        assert (got == SM.merged_reference(plain, exps, n)).all(), exps
        # the raw output: twist left in, so the plain transform gives the table on LDE coset 1
        for t in range(3):
            assert (ref.O.ntt(raw[t]) == ref.values_of_vector(plain[0, t], 1)).all()


@pytest.mark.parametrize("n", [64, 256])
def test_merge_constants_give_the_monomial(ref, n):
    """c[i][wrapped] are the factors of the rotated vector: for a single term, rotating the plain vector and scaling it is the merged
    reference -- for both bases and both first cosets"""
    rng = np.random.default_rng(n + 2)
    d_in = random_words(ref, rng, 1, 4, n)
    plain = ref.even_to_odd(d_in)[:, 0]
    for e in (0, 1, n - 1, n, 8 * n + 1, 16 * n - 1, 2**40 + 3):
        c, r = ref.merge_constants(e, n)
        assert r == e % n
        want, _ = ref.merged(d_in, [[(0, e)]])
        for kc in range(4):
            s = ref.ints(plain[kc])
            assert ref.ints(want[kc, 0]) == [c[kc][1 if q < r else 0] * s[(q - r) % n] % P for q in range(n)], (e, kc)
    # k0 = 2, base g w_8n: the term k_final_hi_merge consumes
    base = G * ref.root(n.bit_length() + 2) % P
    tco, qco = random_words(ref, rng, 1, 2, n), random_words(ref, rng, 1, 2, n)
    h = [ref.ints(v) for v in ref.halved_difference(tco, qco)[0]]
    for e in (n - 1, 8 * n + 1, 5 * n + 3):
        c, r = ref.merge_constants(e, n, base, 2)
        want = ref.final_hi_merge(tco, qco, e, base, 2)
        for i in range(3):
            assert ref.ints(want[i, 0]) == [(h[0][q] + c[i][1 if q < r else 0] * h[1][(q - r) % n]) % P for q in range(n)], (e, i)


@pytest.mark.parametrize("log_b", [1, 2, 3])
@pytest.mark.parametrize("n", [64, 256])
def test_coset_combine_reference(ref, n, log_b):
    bb = 1 << log_b
    rng = np.random.default_rng(n + log_b)
    a = random_words(ref, rng, bb * n)
    d_b = ref.combine_inputs(a, log_b)
    assert (ref.combine(d_b) == a).all()
    # closed form: a_(q + n i) = (1 / B) sum_k w_B^(-k i) w_N^(-k q) B_k[q]
    wN = ref.root(n.bit_length() - 1 + log_b)
    b_int = [ref.ints(v) for v in d_b]
    inv_b = pow(bb, -1, P)
    for i in range(bb):
        for q in (0, 1, n // 2 + 1, n - 1):
            assert ref.ints(a[q + n * i:q + n * i + 1])[0] == inv_b * sum(pow(wN, -(k * n * i + k * q), P) * b_int[k][q] for k in range(bb)) % P
    # the oracle's composition stage rests on the same coefficients: H(x) = sum_i x^i H_i(x^B) with x = g y
    vals = np.stack([ref.O.ntt(v) for v in d_b])              # coset-major values over g <w_N>
    cols = ref.O.composition_columns(vals)
    c = ref.scale(a, pow(G, -1, P))
    assert (cols == c.reshape(n, bb).T).all()


def test_final_hi_and_shard_combine_references(ref):
    n = 8
    rng = np.random.default_rng(3)
    odd, direct = random_words(ref, rng, 26, n), random_words(ref, rng, 4, n)
    hi = ref.final_hi(odd, direct, 11, 2, 13)
    two = ref.mont([2])[0]
    for r, table in enumerate((11, 12, 24, 25)):
        assert (ref.O.fp_add(ref.O.fp_mul(hi[r], np.full(n, two, np.uint64)), direct[r]) == odd[table]).all()
    for nkc in (1, 2):
        parts = random_words(ref, rng, 4 // nkc, nkc + 4, n)
        out = ref.shard_combine(parts, nkc)
        for kc in range(4):
            assert (out[2 * kc] == parts[kc // nkc, kc % nkc]).all()
            assert (out[2 * kc + 1] == K.add_mod_p(ref, [parts[r, nkc + kc] for r in range(4 // nkc)])).all()
