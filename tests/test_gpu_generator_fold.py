"""The generator addition folded into the doubling kernel (csrc/generator_fold.h; csrc/constraints.hip: k_ec_split<PART_DBL0>,
k_schnorr_ec_split<PART_DBL0>): the stage on tables that no witness produces.  The fold rests on a polynomial identity in (X, Y, Z)
and on the linearity of the sums in the coefficients, so it must hold off the curve and with a bit register that is not binary:
the tables here are extensions of fully random traces (every column of degree < n, which is all the split evaluation relies on).
Exact field arithmetic: every comparison is bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEPTH = 3


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def random_trace(oracle, width, n, seed):
    return oracle.to_mont(np.random.default_rng(seed).integers(0, oracle.P, size=(width, n), dtype=np.uint64))


def extension(oracle, trace):
    return oracle.lde_columns(oracle.interpolate_columns(trace), 3)


@pytest.fixture(scope="module")
def tx_tables(oracle):
    """name -> (lde [8][94][n], public inputs): random 94 x n traces at n = 1024 and 2048; at n = 1024 also with registers 0..18 (the
    point s*G and its bit) set column-wise to 0, to p - 1, and to 0 / p - 1 alternating from register to register"""
    zero, minus_one = np.uint64(0), oracle.to_mont(np.array([oracle.P - 1], np.uint64))[0]
    tables = {}
    for n in (1024, 2048):
        tables["random_%d" % n] = random_trace(oracle, 94, n, 4000 + n)
    base = tables["random_1024"]
    for name, fill in (("zero", lambda r: zero), ("minus_one", lambda r: minus_one), ("alternating", lambda r: minus_one if r & 1 else zero)):
        t = base.copy()
        for r in range(19):
            t[r, :] = fill(r)
        tables[name] = t
    pub = oracle.random_elements(4, 77)
    return {name: (extension(oracle, t), pub) for name, t in tables.items()}


@pytest.fixture(scope="module")
def coefficient_sets(oracle):
    return [oracle.make_coeffs(700 + q) for q in range(3)]


@pytest.fixture(scope="module")
def tx_references(oracle, tx_tables, coefficient_sets):
    """(table, coefficient set) -> the oracle's merged evaluations at all 8n points, computed once"""
    refs = {}
    for name, (lde, pub) in tx_tables.items():
        for q in range(3 if name.startswith("random") else 1):
            refs[(name, q)] = oracle.tx_evaluate_constraints(lde, coefficient_sets[q], pub, DEPTH, 3)
    return refs


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [1024, 2048])
def test_stage_on_the_extension_of_a_random_trace(backend, tx_tables, coefficient_sets, tx_references, n, m):
    """evaluate_constraints(..., input_is_lde=True) == oracle.tx_evaluate_constraints at all 8n points, for one, two and three
    coefficient sets: points off the curve, register 18 not binary."""
    from certificate_stark_amd.backend import to_numpy_u64
    name = "random_%d" % n
    lde, pub = tx_tables[name]
    d_lde = backend.from_numpy_u64(lde)
    if m == 1:
        got = to_numpy_u64(backend.evaluate_constraints(d_lde, coefficient_sets[0], pub, DEPTH, input_is_lde=True))[None]
    else:
        got = to_numpy_u64(backend.evaluate_constraints_ext(d_lde, coefficient_sets[:m], pub, DEPTH, input_is_lde=True))
    assert got.shape == (m, 8, n)
    for q in range(m):
        ref = tx_references[(name, q)]
        assert (got[q] == ref).all(), "coefficient set %d: cosets that differ: %s" % (q, sorted(set(np.argwhere(got[q] != ref)[:, 0].tolist())))


@pytest.mark.parametrize("fill", ["zero", "minus_one", "alternating"])
def test_stage_with_the_point_registers_at_the_operand_extremes(backend, tx_tables, coefficient_sets, tx_references, fill):
    """the same at n = 1024 with registers 0..18 constant: all 0, all p - 1, 0 and p - 1 alternating by register"""
    from certificate_stark_amd.backend import to_numpy_u64
    lde, pub = tx_tables[fill]
    got = to_numpy_u64(backend.evaluate_constraints(backend.from_numpy_u64(lde), coefficient_sets[0], pub, DEPTH, input_is_lde=True))
    ref = tx_references[(fill, 0)]
    assert got.shape == ref.shape == (8, 1024)
    assert (got == ref).all(), "cosets that differ: %s" % sorted(set(np.argwhere(got != ref)[:, 0].tolist()))


@pytest.mark.parametrize("n_sig", [2, 8])
def test_schnorr_split_equals_direct_evaluation_on_a_random_trace(oracle, backend, n_sig):
    """cstark_schnorr_evaluate_constraints_lde == cstark_schnorr_evaluate_constraints at every point when the 56-register table is the
    extension of a random trace; aux and the assertion polynomials are those of a real witness.  (The degree-split form starts at 8
    signatures, n = 4096; at 2 signatures both entry points evaluate every point directly.)"""
    import torch
    log_b = 3
    w = oracle.SchnorrWitness.generate(n_sig, seed=500 + n_sig)
    backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s)
    log_n = 9 + n_sig.bit_length() - 1
    lde = backend.from_numpy_u64(extension(oracle, random_trace(oracle, 56, 1 << log_n, 6000 + n_sig)))
    aux = backend.lde_columns(backend.interpolate_columns(backend.schnorr_aux_columns()), log_b)
    av = backend.lde_columns(backend.schnorr_assertion_polys(log_n), log_b)
    ta, tb = oracle.random_elements(56, 41), oracle.random_elements(56, 42)
    ba, bb = oracle.random_elements(61, 43), oracle.random_elements(61, 44)
    direct = backend.schnorr_evaluate_constraints(lde, aux, ta, tb, ba, bb, av, log_b, n_sig=n_sig)
    split = backend.schnorr_evaluate_constraints_lde(lde, aux, ta, tb, ba, bb, av, n_sig=n_sig)
    assert direct.shape == split.shape and bool(direct.any())
    assert torch.equal(direct, split)
