"""GPU parity at operand extremes: the kernels that skip full reductions (fp_mul_lazy / fp_inv_sbox, the matrix-core section sums of
rounds_mfma.hip and mds_mfma.cuh, the wide accumulators of the curve formulas) fed the values where their hand-derived bounds are
tight -- 0, p - 1, (p-1)/2, (p+1)/2, the Montgomery one and the cube roots that put cube(x) there -- instead of uniform random
elements.  Every comparison is bit-exact, against the oracle or against Python integers."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_bounds_model import HALF_P, INV_ALPHA, P, R_INV, inv_sbox_extremes, mul_lazy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 2**64


def mont(x):
    return x * R % P


def canon(x):
    return x * R_INV % P


INV3 = pow(3, -1, P - 1)       # 3 does not divide p - 1: cubing is a bijection of the field


def cube_root_word(t):
    """the memory-form word y with fp_cube(y) == t (fp_cube(y) = y^3 / R^2 on words)"""
    return mont(pow(canon(t), INV3, P))


CUBE_TARGETS = [0, P - 1, HALF_P - 1, HALF_P, HALF_P + 1]
EXT = [0, P - 1, HALF_P, HALF_P + 1, mont(1)]
EXT_ALL = EXT + [cube_root_word(t) for t in CUBE_TARGETS]


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _fp_op(backend, a, b, op):
    from certificate_stark_amd import _lib
    from certificate_stark_amd.backend import to_numpy_u64
    a = np.ascontiguousarray(a, np.uint64)
    da = backend.from_numpy_u64(a)
    db = backend.from_numpy_u64(np.ascontiguousarray(b, np.uint64)) if b is not None else None
    out = backend.empty_u64(a.size)
    rc = _lib.load_debug().cstark_debug_fp_op(C.c_void_p(backend.stream.cuda_stream), backend._ptr(da),
                                              backend._ptr(db) if db is not None else None, backend._ptr(out), C.c_size_t(a.size), C.c_int(op))
    assert rc == 0
    backend.synchronize()
    return to_numpy_u64(out)


# ---- 1. field primitives at their bounds ----------------------------------------------------------------------------------------

def test_raw_lazy_product_for_factors_in_p_2p_and_at_the_high_word_limit(backend):
    """fp_mul_lazy with no final subtraction (debug op 13) equals the word-exact model for every pair; where no sum wraps (both
    factors below 2p, or a second factor's high word up to 0xBE7FFFFE) it is congruent to a b 2^-64 and at most a b / 2^64 + p + p / 2^32"""
    rng = random.Random(13)
    big = [P, P + 1, P + 2, P + 2**32, 2 * P - 1, 2 * P - 2, 2 * P - 2**32, P + HALF_P, (3 * P) // 2]
    big += [rng.randrange(P, 2 * P) for _ in range(40)]
    a = [x for x in big for _ in big]
    b = [y for _ in big for y in big]
    # second factors whose high word sits at the c-sum limit, first factors with an all-ones low word (the largest w >> 32)
    for b1 in (0xBE7FFFFC, 0xBE7FFFFD, 0xBE7FFFFE, 0xBE7FFFFF):
        for lo in (0, 1, 2**32 - 1, 0x80000000, rng.randrange(2**32)):
            for a_ in ((rng.randrange(2**31) << 32) | (2**32 - 1) for _ in range(8)):
                a.append(a_)
                b.append((b1 << 32) | lo)
    a, b = np.array(a, np.uint64), np.array(b, np.uint64)
    got = _fp_op(backend, a, b, 13)
    want, wrapped = mul_lazy(a, b)
    assert (got == want).all()
    nw = 0
    for x, y, r, w in zip(a.tolist(), b.tolist(), got.tolist(), wrapped.tolist()):
        if w:
            assert y >> 32 == 0xBE7FFFFF          # only past the limit
            continue
        nw += 1
        assert r % P == x * y * R_INV % P
        assert r * R <= x * y + P * (R + 2**32)
    assert nw > len(big) ** 2


def test_cube_and_inverse_sbox_at_the_edges(backend):
    """fp_cube (op 14) and fp_inv_sbox (op 4) against pow() in Python integers on the edge set and the cube roots of the edges"""
    words = sorted(set(EXT_ALL + [1, 2, P - 2, 2**32 - 1, 2**32, 2**62, P - 2**32, HALF_P - 1] + [cube_root_word(t) for t in EXT]))
    a = np.array(words, np.uint64)
    cubes = _fp_op(backend, a, None, 14)
    for x, c in zip(words, cubes.tolist()):
        assert c == mont(pow(canon(x), 3, P)), hex(x)
    for t in CUBE_TARGETS:
        assert cubes[words.index(cube_root_word(t))] == t
    inv = _fp_op(backend, a, None, 4)
    for x, r in zip(words, inv.tolist()):
        assert r == mont(pow(canon(x), INV_ALPHA, P)), hex(x)


def test_inverse_sbox_on_the_inputs_that_drive_its_lazy_chain_highest(backend):
    """the 4096 inputs (of 2^20 candidates, selected on the word-exact model) whose unreduced chain climbs highest"""
    xs, hi = inv_sbox_extremes(k=4096)
    assert int(hi[0]) > 1.5 * P
    got = _fp_op(backend, xs, None, 4)
    for x, r in zip(xs.tolist(), got.tolist()):
        assert r == mont(pow(canon(x), INV_ALPHA, P)), hex(x)


def _header_matrix(name):
    txt = open(os.path.join(ROOT, "oracle", "constants_gen.h")).read()
    body = txt[txt.index("#define %s_INIT" % name):]
    body = body[body.index("{") + 1:body.index("}")]
    return [int(t.strip().rstrip("ULul"), 0) for t in body.replace("\\", " ").split(",") if t.strip()]


def _digit_vector(pattern):
    """a field element whose bytes 0..6 give the matrix-core operand digit `pattern` (x = s + X0: byte 0x00 -> -128, 0xff -> +127)"""
    lo = sum(b << (8 * i) for i, b in enumerate(pattern))
    return (0x40 << 56) | lo


@pytest.mark.parametrize("use_mfma", [0, 1])
def test_inverse_mds_product_at_digit_extremes(backend, use_mfma):
    """cstark_debug_mds (INV_MDS v on the matrix cores or by limb dot products) against Python integers: sum_j M_ij v_j 2^-64 mod p,
    for vectors whose operand digits are all -128, all +127 or alternating, and 0, p - 1, (p-1)/2, (p+1)/2"""
    from certificate_stark_amd import _lib
    from certificate_stark_amd.backend import to_numpy_u64
    M = _header_matrix("CS_INV_MDS_MONT")
    assert len(M) == 196
    vals = [0, P - 1, HALF_P, HALF_P + 1, _digit_vector([0x00] * 7), _digit_vector([0xff] * 7), _digit_vector([0x00, 0xff] * 3 + [0x00]),
            _digit_vector([0xff, 0x00] * 3 + [0xff]), (0x41 << 56) | 0x7fffffffffffff, 0x4180000000000000]
    assert all(v < P for v in vals)
    rng = random.Random(21)
    npts = 512
    vecs = [[v] * 14 for v in vals]
    vecs += [[vals[(i + s) % len(vals)] for i in range(14)] for s in range(len(vals))]
    vecs += [[rng.choice(vals) for _ in range(14)] for _ in range(npts - len(vecs))]
    inp = np.array(vecs, np.uint64).T.copy()          # [14][npts]
    d_in, d_out = backend.from_numpy_u64(inp), backend.empty_u64(14, npts)
    ms = C.c_float()
    rc = _lib.load_debug().cstark_debug_mds(C.c_void_p(backend.stream.cuda_stream), backend._ptr(d_in), backend._ptr(d_out), C.c_size_t(npts),
                                            C.c_int(use_mfma), C.c_int(1), C.byref(ms))
    assert rc == 0
    backend.synchronize()
    got = to_numpy_u64(d_out)
    for pt, v in enumerate(vecs):
        for i in range(14):
            assert int(got[i, pt]) == sum(M[i * 14 + j] * v[j] for j in range(14)) * R_INV % P, (pt, i)


# ---- 2. the production (degree-split) constraint path on degenerate traces -------------------------------------------------------

def _const_lde(values, n):
    """the LDE of a trace whose column c is the constant values[c]: that constant at every point of all 8 cosets"""
    return np.ascontiguousarray(np.broadcast_to(np.array(values, np.uint64)[None, :, None], (8, 94, n)))


def _coeffs(t_alpha, t_beta, b_alpha, b_beta):
    from certificate_stark_amd._lib import TxCoeffsStruct
    cf = TxCoeffsStruct()
    for name, v in (("t_alpha", t_alpha), ("t_beta", t_beta), ("b_alpha", b_alpha), ("b_beta", b_beta)):
        for i, x in enumerate(v):
            getattr(cf, name)[i] = int(x)
    return cf


def _extreme_coeff_sets(oracle):
    z115, z4 = [0] * 115, [0] * 4
    one_t = [0] * 115
    one_t[3] = HALF_P + 1
    one_b = [0] * 4
    one_b[2] = P - 1
    rnd = oracle.make_coeffs(29)
    return {"random": _coeffs(*[list(getattr(rnd, f)) for f in ("t_alpha", "t_beta", "b_alpha", "b_beta")]),
            "alpha=(p-1)/2": _coeffs([HALF_P] * 115, z115, [HALF_P] * 4, z4),
            "alpha=(p+1)/2": _coeffs([HALF_P + 1] * 115, z115, [HALF_P + 1] * 4, z4),
            "beta=p-1": _coeffs([P - 1] * 115, [P - 1] * 115, [P - 1] * 4, [P - 1] * 4),
            "one transition": _coeffs(one_t, z115, z4, z4),
            "one boundary": _coeffs(z115, z115, one_b, z4)}


def _degenerate_traces(n):
    cols = {"zero": [0] * 94}
    for v in EXT_ALL[1:]:
        cols["all %#x" % v] = [v] * 94
    for s in range(3):
        cols["mixed %d" % s] = [EXT_ALL[(7 * c + s) % len(EXT_ALL)] for c in range(94)]
    return cols


@pytest.mark.parametrize("log_n,depth", [(10, 3), (11, 15), (12, 7)])
def test_split_constraint_path_on_constant_traces(oracle, backend, log_n, depth):
    """cstark_tx_evaluate_constraints_lde (k_rounds_mfma, k_ec_split, k_lin_all, k_final_split, k_split_finish) is exact for the
    extension of any trace; a trace of constant columns is one, and its extension holds those constants at every point"""
    from certificate_stark_amd.backend import to_numpy_u64
    n = 1 << log_n
    sets = _extreme_coeff_sets(oracle)
    names = list(sets) if log_n == 10 else ["random", "alpha=(p+1)/2", "beta=p-1"]
    for tname, vals in _degenerate_traces(n).items():
        lde = _const_lde(vals, n)
        d_lde = backend.from_numpy_u64(lde)
        for pub in ([0, 0, 0, 0], [P - 1, HALF_P, HALF_P + 1, 0]):
            for cname in names:
                ref = oracle.tx_evaluate_constraints(lde, sets[cname], pub, depth, 3)
                got = to_numpy_u64(backend.evaluate_constraints(d_lde, sets[cname], pub, depth, input_is_lde=True))
                assert (got == ref).all(), (tname, cname, pub)
            if log_n != 10:
                break


def test_split_constraint_path_on_real_traces_with_constant_blocks(oracle, backend):
    """tx_build_trace traces with blocks of columns overwritten by extreme constants (still columns of degree < n)"""
    from certificate_stark_amd.backend import to_numpy_u64
    w = oracle.TxWitness.generate(2, 15, seed=606)
    base = oracle.tx_build_trace(w)
    pub = np.concatenate([w.initial_roots[0][:2], w.final_root[:2]])
    sets = _extreme_coeff_sets(oracle)
    for k, (c0, c1) in enumerate([(0, 14), (14, 28), (28, 56), (56, 94), (0, 94)]):
        t = base.copy()
        t[c0:c1] = np.array([EXT_ALL[(k + c) % len(EXT_ALL)] for c in range(c0, c1)], np.uint64)[:, None]
        lde = oracle.lde_columns(oracle.interpolate_columns(t), 3)
        d_lde = backend.from_numpy_u64(lde)
        for cname in ("random", "alpha=(p+1)/2"):
            ref = oracle.tx_evaluate_constraints(lde, sets[cname], pub, 15, 3)
            got = to_numpy_u64(backend.evaluate_constraints(d_lde, sets[cname], pub, 15, input_is_lde=True))
            assert (got == ref).all(), ((c0, c1), cname)


@pytest.mark.parametrize("m", [2, 3])
def test_split_path_with_several_coefficient_sets_on_constant_traces(oracle, backend, m):
    """the extension-field proof's split path (cstark_tx_evaluate_constraints_ext_lde): every set equals its oracle evaluation"""
    from certificate_stark_amd.backend import to_numpy_u64
    n, depth = 1 << 11, 15
    sets = list(_extreme_coeff_sets(oracle).values())
    for s in range(3):
        vals = _degenerate_traces(n)["mixed %d" % s] if s else [HALF_P + 1] * 94
        lde = _const_lde(vals, n)
        chosen = [sets[(s + q) % len(sets)] for q in range(m)]
        pub = [P - 1, 0, HALF_P, 1]
        got = to_numpy_u64(backend.evaluate_constraints_ext(backend.from_numpy_u64(lde), chosen, pub, depth, input_is_lde=True))
        assert got.shape == (m, 8, n)
        for q in range(m):
            assert (got[q] == oracle.tx_evaluate_constraints(lde, chosen[q], pub, depth, 3)).all(), (s, q)


# ---- 3. direct evaluators on arbitrary extreme tables ---------------------------------------------------------------------------

def _extreme_table(shape, seed):
    rng = np.random.default_rng(seed)
    return np.array(EXT_ALL, np.uint64)[rng.integers(0, len(EXT_ALL), size=shape)]


def test_tx_direct_evaluators_on_extreme_tables(oracle, backend):
    """evaluate_transitions and evaluate_constraints are exact for any table: every cell drawn from the extreme set"""
    from certificate_stark_amd.backend import to_numpy_u64
    sets = _extreme_coeff_sets(oracle)
    for seed, depth in ((1, 15), (2, 3)):
        lde = _extreme_table((8, 94, 1024), seed)
        d_lde = backend.from_numpy_u64(lde)
        got = to_numpy_u64(backend.evaluate_transitions(d_lde, depth))
        assert (got == oracle.tx_evaluate_transitions(lde, depth, 3)).all()
        for cname in ("random", "alpha=(p-1)/2", "alpha=(p+1)/2"):
            ref = oracle.tx_evaluate_constraints(lde, sets[cname], [P - 1, 0, HALF_P, 1], depth, 3)
            got = to_numpy_u64(backend.evaluate_constraints(d_lde, sets[cname], [P - 1, 0, HALF_P, 1], depth))
            assert (got == ref).all(), cname


def _merkle_case(oracle, seed):
    w = oracle.TxWitness.generate(2, 7, seed=seed)
    desc = oracle.merkle_desc(oracle.merkle_build_trace(w))
    lde = _extreme_table((8, 65, 1024), seed)
    ta, tb = [HALF_P + 1] * 106, [0] * 106
    ba, bb = oracle.random_elements(14, 3), [P - 1] * 14
    ev = oracle.air_evaluate_transitions(oracle.AIR_MERKLE, lde, oracle.periodic_table(oracle.merkle_periodic_columns(7), 10, 3), 106)
    ref = oracle.air_combine(desc, lde, ev, ta, tb, ba, bb, 3)
    return lde, (ta, tb, ba, bb, desc.a_value), ref


def test_merkle_fused_evaluator_on_extreme_tables(oracle, backend):
    """cstark_merkle_evaluate_constraints (k_merkle_rounds_mfma: n % 256 == 0) on extreme tables, against transitions + combine"""
    from certificate_stark_amd.backend import to_numpy_u64
    for seed in (5, 6):
        lde, (ta, tb, ba, bb, av), ref = _merkle_case(oracle, seed)
        got = to_numpy_u64(backend.merkle_evaluate_constraints(backend.from_numpy_u64(lde), 7, ta, tb, ba, bb, av, 3))
        assert (got == ref).all()


def test_schnorr_fused_evaluator_on_extreme_tables(oracle, backend):
    """cstark_schnorr_evaluate_constraints (the curve formulas' lazy tower arithmetic) with trace and aux tables of extreme cells"""
    from certificate_stark_amd.backend import to_numpy_u64
    n_sig, log_b = 2, 3
    w = oracle.SchnorrWitness.generate(n_sig, seed=8)
    log_n = 10
    desc = oracle.schnorr_desc(w)
    avals = oracle.lde_columns(oracle.schnorr_assertion_polys(w, log_n), log_b)
    ptab = oracle.periodic_table(oracle.schnorr_mask_columns(), log_n, log_b)
    for seed in (9, 10):
        lde, aux = _extreme_table((8, 56, 1024), seed), _extreme_table((8, 19, 1024), seed + 100)
        ta, tb = [HALF_P + 1] * 56, oracle.random_elements(56, seed)
        ba, bb = [HALF_P] * 61, [0] * 61
        ev = oracle.schnorr_evaluate_transitions(lde, aux, ptab)
        ref = oracle.air_combine(desc, lde, ev, ta, tb, ba, bb, log_b, avals=avals)
        got = to_numpy_u64(backend.schnorr_evaluate_constraints(backend.from_numpy_u64(lde), backend.from_numpy_u64(aux), ta, tb, ba, bb,
                                                                backend.from_numpy_u64(avals), log_b, n_sig=n_sig))
        assert (got == ref).all(), seed


MERKLE_WINDOW_REGS = (0, 15, 29, 44)   # c_windows of rounds_layout.h: the four Rescue windows of MerkleAir's 65-register frame


def _merkle_section_limit_table(oracle, seed, sign):
    """A Merkle table whose alpha round sections sit at their bound on every even point, all 28 products of a section at their
    extreme with the same sign: alpha coefficients (p+1)/2 (centred -(p-1)/2; sign +1) or (p-1)/2 (sign -1), next = MDS y + ark2(point)
    with y = 0 so that every cube(y) is 0, and cur chosen per entry so that cube(cur) is 0 or p - 1 to match the sign of the folded
    coefficient -U = -(MDS^T gamma).  Returns the table, the coefficients and the extreme section value (the integer fed to acc_fold /
    acc_reduce) over all windows."""
    from test_bounds_model import section_value
    lde, (_, tb, ba, bb, av), _ = _merkle_case(oracle, seed)
    ta = [HALF_P + 1 if sign > 0 else HALF_P] * 106
    mds = _header_matrix("CS_MDS_MONT")
    ptab = oracle.periodic_table(oracle.merkle_periodic_columns(7), 10, 3)      # [8][33][512]; ark2 = columns 5 + 14 ..
    n = lde.shape[2]
    values = []
    for reg in MERKLE_WINDOW_REGS:
        gam = ta[reg:reg + 14]
        c = [(P - sum(gam[i] * mds[i * 14 + t] for i in range(14)) * R_INV % P) % P for t in range(14)]
        # product sign: sign(centred c) * sign(cube - (p-1)/2 - X0), negative for cube = 0, positive for cube = p - 1
        cube_t = [P - 1 if (1 if x <= HALF_P else -1) == sign else 0 for x in c]
        cur = [0 if y == 0 else cube_root_word(P - 1) for y in cube_t]
        values.append(section_value(gam + c, [0] * 14 + cube_t)[0])
        for k in range(8):
            for j in range(0, n, 2):
                lde[k, reg:reg + 14, j] = cur
                lde[k, reg:reg + 14, j + 1] = ptab[k, 19:33, j % 512]
    return lde, (ta, tb, ba, bb, av), (max(values) if sign > 0 else min(values))


@pytest.mark.parametrize("sign", [1, -1])
def test_merkle_round_sections_forced_to_their_limit(oracle, backend, sign):
    """both halves of every Merkle alpha section at the extreme at once (k_merkle_rounds_mfma), against transitions + combine.  The
    centred sum reaches 0.67 of its 7.11 p^2 bound either way: section values 0.82 and 0.20 of 2^128 around the 2p 2^64 offset (0.51),
    where random data stays within about 2^123 of it.  The low side is below p 2^64: a smaller offset would wrap."""
    from certificate_stark_amd.backend import to_numpy_u64
    lde, (ta, tb, ba, bb, av), v = _merkle_section_limit_table(oracle, 5, sign)
    assert 0 <= v < 2**128
    assert (v > 0.8 * 2**128) if sign > 0 else (v < P * 2**64)
    ptab = oracle.periodic_table(oracle.merkle_periodic_columns(7), 10, 3)
    ev = oracle.air_evaluate_transitions(oracle.AIR_MERKLE, lde, ptab, 106)
    w = oracle.TxWitness.generate(2, 7, seed=5)
    ref = oracle.air_combine(oracle.merkle_desc(oracle.merkle_build_trace(w)), lde, ev, ta, tb, ba, bb, 3)
    got = to_numpy_u64(backend.merkle_evaluate_constraints(backend.from_numpy_u64(lde), 7, ta, tb, ba, bb, av, 3))
    assert (got == ref).all()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from certificate_stark_amd.backend import Backend, to_numpy_u64
from certificate_stark_amd._lib import TxCoeffsStruct
z = np.load(%(path)r)
b = Backend()
cf = TxCoeffsStruct()
for name in ("t_alpha", "t_beta", "b_alpha", "b_beta"):
    for i, x in enumerate(z[name]):
        getattr(cf, name)[i] = int(x)
got = to_numpy_u64(b.evaluate_constraints(b.from_numpy_u64(z["tx_lde"]), cf, z["pub"], 15))
assert (got == z["tx_ref"]).all(), "tx evaluate_constraints"
m = z["mk_args"]
got = to_numpy_u64(b.merkle_evaluate_constraints(b.from_numpy_u64(z["mk_lde"]), 7, m[0, :106], m[1, :106], m[2, :14], m[3, :14], m[4, :14], 3))
assert (got == z["mk_ref"]).all(), "merkle_evaluate_constraints"
b.close()
print("vector-alu ok")
"""


def test_vector_alu_fallbacks_on_extreme_tables(oracle, tmp_path):
    """the same extreme tables through the vector-ALU kernels (CSTARK_ROUNDS_MFMA=0 is read once per process: a child process)"""
    cf = _extreme_coeff_sets(oracle)["alpha=(p+1)/2"]
    tx_lde = _extreme_table((8, 94, 1024), 1)
    pub = np.array([P - 1, 0, HALF_P, 1], np.uint64)
    tx_ref = oracle.tx_evaluate_constraints(tx_lde, cf, pub, 15, 3)
    mk_lde, (ta, tb, ba, bb, av), mk_ref = _merkle_case(oracle, 5)
    mk_args = np.zeros((5, 106), np.uint64)
    for r, v in enumerate((ta, tb, ba, bb, av)):
        mk_args[r, :len(v)] = np.array(v, np.uint64)
    path = str(tmp_path / "extreme_tables.npz")
    np.savez(path, tx_lde=tx_lde, tx_ref=tx_ref, pub=pub, mk_lde=mk_lde, mk_ref=mk_ref, mk_args=mk_args,
             **{name: np.array(list(getattr(cf, name)), np.uint64) for name in ("t_alpha", "t_beta", "b_alpha", "b_beta")})
    got = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "path": path}], env=dict(os.environ, CSTARK_ROUNDS_MFMA="0"),
                         capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout.strip().splitlines()[-1] == "vector-alu ok"


# ---- 4. degenerate witnesses through trace generation ---------------------------------------------------------------------------

def _hand_witness(oracle, n_tx, depth, fill, idx, delta, sig_s, sig_rx):
    w = oracle.TxWitness(n_tx, depth)
    for f in ("initial_roots", "final_root", "s_old_values", "r_old_values", "s_paths", "r_paths"):
        getattr(w, f)[...] = fill
    w.s_indices[...] = idx
    w.r_indices[...] = (2**depth - 1) - idx
    w.deltas[...] = delta
    w.sig_s[...] = np.frombuffer(sig_s.to_bytes(32, "little"), np.uint8)
    w.sig_rx[...] = sig_rx
    return w


@pytest.mark.parametrize("depth", [3, 15])
def test_trace_generation_on_degenerate_witnesses(oracle, backend, depth):
    """hand-filled TxWitness objects (zero / p - 1 values, paths and roots; indices 0 and 2^depth - 1; deltas 0 and p - 1; sig_s all
    0x00, all 0xff and 2^255 +- 1 -- the curve order is not known to the reference, 2^255 is the bound its signer keeps s under; sig_rx
    zero): the GPU trace equals the oracle's.  Parity, not validity."""
    from certificate_stark_amd.backend import to_numpy_u64
    cases = [(0, 0, 0, 0, 0), (P - 1, 2**depth - 1, P - 1, 2**256 - 1, 0), (HALF_P + 1, 0, P - 1, 2**255 - 1, P - 1),
             (P - 1, 2**depth - 1, 0, 2**255 + 1, HALF_P), (mont(1), 0, HALF_P, 2**255, 0)]
    for k, (fill, idx, delta, s, rx) in enumerate(cases):
        w = _hand_witness(oracle, 2, depth, fill, idx, delta, s, rx)
        ref = oracle.tx_build_trace(w)
        backend.upload_witness(w)
        got = to_numpy_u64(backend.build_trace())
        if not (got == ref).all():
            raise AssertionError("case %d: columns differ %s" % (k, sorted(set(np.argwhere(got != ref)[:, 0].tolist()))))


def test_schnorr_trace_generation_on_degenerate_witnesses(oracle, backend):
    from certificate_stark_amd.backend import to_numpy_u64
    for k, (msg, rx, s) in enumerate([(0, 0, 0), (P - 1, 0, 2**256 - 1), (HALF_P, P - 1, 2**255 - 1), (mont(1), HALF_P + 1, 2**255 + 1)]):
        w = oracle.SchnorrWitness(2)
        w.messages[...] = msg
        w.sig_rx[...] = rx
        w.sig_s[...] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
        backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s)
        got = to_numpy_u64(backend.schnorr_build_trace())
        ref = oracle.schnorr_build_trace(w)
        if not (got == ref).all():
            raise AssertionError("case %d: columns differ %s" % (k, sorted(set(np.argwhere(got != ref)[:, 0].tolist()))))
        assert (to_numpy_u64(backend.schnorr_aux_columns()) == oracle.schnorr_aux_columns(w)).all(), k


# ---- 5. transforms and tail -------------------------------------------------------------------------------------------------------

def _extreme_columns(n):
    spike = np.zeros(n, np.uint64)
    spike[n // 3] = P - 1
    return np.stack([np.full(n, P - 1, np.uint64), np.tile(np.array([0, P - 1], np.uint64), n // 2), np.full(n, HALF_P, np.uint64), spike])


@pytest.mark.parametrize("log_n", [16, 18, 20])
def test_interpolation_and_lde_on_extreme_columns(oracle, backend, log_n):
    """the large-size transform kernels on columns all p - 1, alternating 0 / p - 1, all (p-1)/2 and a single p - 1 spike"""
    from certificate_stark_amd.backend import to_numpy_u64
    ev = _extreme_columns(1 << log_n)
    co_ref = oracle.interpolate_columns(ev)
    co = backend.interpolate_columns(backend.from_numpy_u64(ev))
    assert (to_numpy_u64(co) == co_ref).all()
    log_b, nk = (3, None) if log_n < 20 else (3, 2)
    lde_ref = oracle.lde_columns(co_ref, log_b, nk=nk)
    assert (to_numpy_u64(backend.lde_columns(co, log_b, nk=nk)) == lde_ref).all()


@pytest.mark.parametrize("folding", [4, 8, 16])
def test_fri_folding_on_extreme_evaluations(oracle, backend, folding):
    from certificate_stark_amd.backend import to_numpy_u64
    N = 1 << 12
    offset = oracle.generator()
    for ev in (np.full(N, P - 1, np.uint64), np.tile(np.array([0, P - 1], np.uint64), N // 2)):
        d_ev = backend.from_numpy_u64(ev)
        for alpha in (0, mont(1), P - 1, HALF_P + 1):
            got = to_numpy_u64(backend.fri_fold(d_ev, offset, alpha, folding))
            assert (got == oracle.fri_fold(ev, offset, alpha, folding)).all(), alpha
        for m in (2, 3):
            evm = np.ascontiguousarray(np.stack([ev] * m))
            for alpha in ([0] * m, [P - 1] * m, [mont(1)] + [0] * (m - 1)):
                got = to_numpy_u64(backend.fri_fold_ext(backend.from_numpy_u64(evm), offset, alpha, folding))
                assert (got == oracle.fri_fold_ext(evm, offset, np.array(alpha, np.uint64), folding)).all(), (m, alpha)


def test_composition_columns_on_extreme_input(oracle, backend):
    from certificate_stark_amd.backend import to_numpy_u64
    for comb in (np.full((8, 1 << 11), P - 1, np.uint64), _extreme_table((8, 1 << 11), 3)):
        got = to_numpy_u64(backend.composition_columns(backend.from_numpy_u64(comb)))
        assert (got == oracle.composition_columns(comb)).all()
