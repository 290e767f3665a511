"""The degree-split constraint stage with its flag families merged BEFORE the odd-coset transforms (csrc/ntt.h:
coset_even_to_odd_merged; CSTARK_SPLIT_MERGE=0 keeps one transform per polynomial).  Multiplying a polynomial by x^e rotates its
coefficient vector by e mod n and multiplies the wrapped entries by y^n, so a family sum_t x^(e_t) S_t becomes one input vector per
odd coset.  Everything here is exact field arithmetic: every comparison is bit for bit."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**62 + 2**56 + 2**55 + 1
G = 3                                 # LDE offset = the field's generator (include/cstark_conventions.h)
W8 = pow(G, (P - 1) // 8, P)          # the 8th root of unity get_root_of_unity(3): generator^((p - 1) / 2^55) squared 52 times
GROUP_BASE, GROUP_CYCLES = (5, 4, 3), (2, 2, 1)   # degree groups 0..2 of TransactionAir (csrc/constraints.h)


def group_adjustment(g, n):
    """csrc/air_tx_host.h, tx_group_adjustment for the 8n-point domain: (8n - 1) + (n - 1) - evaluation degree of the group"""
    return (8 * n - 1) + (n - 1) - (GROUP_BASE[g] * (n - 1) + GROUP_CYCLES[g] * (n // 1024) * 1023)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------

N = 1024
EXPONENT_SETS = [
    (3 * N, N + 1, 2 * N - 1),             # r = 0 with d = 3 | r = 1 | r = n - 1
    (8 * N + 5, 1, 10 * N - 1),            # e > 8n (d wraps mod 8) | d = 0, r = 1 | d = 9, r = n - 1
    (N - 1, 13 * N + 700, 5 * N),          # d = 0, r = n - 1 | e > 8n | r = 0 with d = 5
    (group_adjustment(0, N), group_adjustment(1, N), group_adjustment(2, N)),  # what the constraint stage uses at this length
]


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(20240)
    return rng.integers(0, P, size=(4, 4, N), dtype=np.uint64)


def merged_reference(plain, exps, n):
    """plain[kc][t][q] = the plain kernel's vectors (memory-form words: the map is linear, so the words themselves are merged with
    canonical constants).  Families {S_0 + x^e0 S_1 + x^e1 S_2}, {x^e2 S_3}; coset k = 2 kc + 1."""
    out = [[[0] * n for _ in range(2)] for _ in range(4)]
    fam = [[(0, 0), (1, exps[0]), (2, exps[1])], [(3, exps[2])]]
    for kc in range(4):
        k = 2 * kc + 1
        for f, terms in enumerate(fam):
            acc = [0] * n
            for t, e in terms:
                d, r = divmod(e, n)
                c0 = pow(G, e, P) * pow(W8, k * d, P) % P
                c1 = c0 * pow(W8, k, P) % P
                s = [int(v) for v in plain[kc][t]]
                for q in range(n):
                    acc[q] = (acc[q] + (c1 if q < r else c0) * s[(q - r) % n]) % P
            out[kc][f] = acc
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("exps", EXPONENT_SETS)
def test_merged_extension_kernel_equals_the_plain_one_merged_in_integers(backend, tables, exps):
    from certificate_stark_amd import _lib
    from certificate_stark_amd.backend import to_numpy_u64
    dbg = _lib.load_debug()
    d_in = backend.from_numpy_u64(tables)
    d_plain, d_merged = backend.empty_u64(4, 4, N), backend.empty_u64(4, 2, N)
    e = (C.c_uint64 * 3)(*exps)
    rc = dbg.cstark_debug_split_merge(C.c_void_p(backend.stream.cuda_stream), backend._ptr(d_in), backend._ptr(d_plain), backend._ptr(d_merged),
                                      C.c_uint32(N.bit_length() - 1), e)
    assert rc == 0
    backend.synchronize()
    plain, merged = to_numpy_u64(d_plain), to_numpy_u64(d_merged)
    assert (plain < np.uint64(P)).all() and plain.any()
    ref = merged_reference(plain, exps, N)
    assert (merged == ref).all(), "cosets x families that differ: %s" % sorted(set(map(tuple, np.argwhere(merged != ref)[:, :2].tolist())))


# ---- 2. the stage against the oracle ---------------------------------------------------------------------------------------------

def assert_adjustments_exercise_the_carry(n):
    """The stage's three exponents at this length: each must rotate (r != 0) and carry (d != 0), and no two may rotate alike --
    otherwise the inputs would not tell a wrong wrap constant or a swapped exponent from a right one."""
    adj = [group_adjustment(g, n) for g in range(3)]
    rs = [a % n for a in adj]
    assert all(rs), "an adjustment is a multiple of n at n = %d: this length does not exercise the rotation" % n
    assert len(set(rs)) == 3, "two adjustments rotate alike at n = %d: this length does not tell the families' exponents apart" % n
    assert all(a // n for a in adj), "an adjustment below n at n = %d: the quotient's factor is not exercised" % n


@pytest.fixture(scope="module")
def stage_cases(oracle):
    """(n_tx, depth) -> [(lde, reference), ...] for the valid and the perturbed trace; coefficients and public inputs alongside"""
    cases = {}
    cf = oracle.make_coeffs(23)
    for n_tx, depth in [(1, 3), (2, 7)]:
        w = oracle.TxWitness.generate(n_tx, depth, seed=91 + n_tx)
        trace = oracle.tx_build_trace(w)
        pub = np.concatenate([w.initial_roots[0][:2], w.final_root[:2]])
        ldes = []
        for perturb in (False, True):
            t = trace.copy()
            if perturb:
                t[17, 5] ^= np.uint64(1)
                t[70, 900] ^= np.uint64(3)
            ldes.append(oracle.lde_columns(oracle.interpolate_columns(t), 3))
        cases[(n_tx, depth)] = (cf, pub, ldes)
    return cases


@pytest.mark.parametrize("n_tx,depth", [(1, 3), (2, 7)])
def test_merged_stage_matches_the_oracle(oracle, backend, stage_cases, n_tx, depth):
    from certificate_stark_amd.backend import to_numpy_u64
    cf, pub, ldes = stage_cases[(n_tx, depth)]
    assert_adjustments_exercise_the_carry(ldes[0].shape[2])
    for lde, what in zip(ldes, ("valid", "perturbed")):
        ref = oracle.tx_evaluate_constraints(lde, cf, pub, depth, 3)
        got = to_numpy_u64(backend.evaluate_constraints(backend.from_numpy_u64(lde), cf, pub, depth, input_is_lde=True))
        assert got.shape == ref.shape == (8, lde.shape[2])
        assert (got == ref).all(), "%s trace: cosets that differ: %s" % (what, sorted(set(np.argwhere(got != ref)[:, 0].tolist())))


@pytest.mark.parametrize("m", [2, 3])
def test_merged_stage_for_several_coefficient_sets(oracle, backend, stage_cases, m):
    from certificate_stark_amd.backend import to_numpy_u64
    _, pub, ldes = stage_cases[(1, 3)]
    lde = ldes[0]
    assert_adjustments_exercise_the_carry(lde.shape[2])
    sets = [oracle.make_coeffs(100 + q) for q in range(m)]
    got = to_numpy_u64(backend.evaluate_constraints_ext(backend.from_numpy_u64(lde), sets, pub, 3, input_is_lde=True))
    assert got.shape == (m, 8, lde.shape[2])
    for q in range(m):
        assert (got[q] == oracle.tx_evaluate_constraints(lde, sets[q], pub, 3, 3)).all(), "coefficient set %d" % q


def test_unmerged_stage_for_several_coefficient_sets(oracle, stage_cases, tmp_path):
    """CSTARK_SPLIT_MERGE=0 with m = 2, 3: the high part's transforms to cosets 3, 5, 7 then read ONE block of 2 m coefficient columns
    for all three cosets.  The switch is read once per process, hence the child, which leaves its outputs in a file."""
    _, pub, ldes = stage_cases[(1, 3)]
    lde = ldes[0]
    assert_adjustments_exercise_the_carry(lde.shape[2])
    np.save(tmp_path / "lde.npy", lde)
    np.save(tmp_path / "pub.npy", pub)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from oracle import oracle as O\n"
            "from certificate_stark_amd.backend import Backend, to_numpy_u64\n"
            "b = Backend()\n"
            "lde, pub = np.load(sys.argv[1] + '/lde.npy'), np.load(sys.argv[1] + '/pub.npy')\n"
            "for m in (2, 3):\n"
            "    sets = [O.make_coeffs(100 + q) for q in range(m)]\n"
            "    got = to_numpy_u64(b.evaluate_constraints_ext(b.from_numpy_u64(lde), sets, pub, 3, input_is_lde=True))\n"
            "    np.save(sys.argv[1] + '/got%%d.npy' %% m, got)\n"
            "b.close()\n") % ROOT
    child = subprocess.run([sys.executable, "-c", code, str(tmp_path)], env=dict(os.environ, CSTARK_SPLIT_MERGE="0"), capture_output=True, text=True,
                           timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    for m in (2, 3):
        got = np.load(tmp_path / ("got%d.npy" % m))
        assert got.shape == (m, 8, lde.shape[2])
        for q in range(m):
            ref = oracle.tx_evaluate_constraints(lde, oracle.make_coeffs(100 + q), pub, 3, 3)
            assert (got[q] == ref).all(), "m = %d, coefficient set %d: cosets that differ: %s" % (m, q, sorted(set(np.argwhere(got[q] != ref)[:, 0].tolist())))


# ---- 3. both paths write the same proof -----------------------------------------------------------------------------------------

def test_merged_and_unmerged_paths_give_the_same_proof_bytes():
    """CSTARK_SPLIT_MERGE is read once per process, hence the child process for the unmerged path.  Both digests are also the CPU
    prover's for the same witness, so that a disagreement between the two says which side wrote the wrong proof."""
    from oracle import oracle as O
    from oracle import prover as OP
    from test_gpu_prove import example
    cpu = hashlib.sha256(OP.prove(O.TxWitness.generate(1, 3, seed=505), (42, 8, 0, 0, 0, 4, 256))).hexdigest()   # example()'s witness and options
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_gpu_prove import example\n"
            "print(hashlib.sha256(example(1, 3, seed=505).prove()).hexdigest())\n") % (ROOT, os.path.join(ROOT, "tests"))
    assert os.environ.get("CSTARK_SPLIT_MERGE", "1") != "0", "this process must run the merged path"
    want = hashlib.sha256(example(1, 3, seed=505).prove()).hexdigest()
    got = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CSTARK_SPLIT_MERGE="0"), capture_output=True, text=True, timeout=600)
    assert got.returncode == 0, got.stderr[-2000:]
    unmerged = got.stdout.strip().splitlines()[-1]
    print("merged %s\nunmerged %s\ncpu %s" % (want, unmerged, cpu))
    assert unmerged == want, "the two paths differ: the merged proof %s the CPU prover's, the unmerged one %s it" % (
        "is" if want == cpu else "is NOT", "is" if unmerged == cpu else "is NOT")
    assert want == cpu, "the merged path (this process) wrote another proof than the CPU prover"
    assert unmerged == cpu, "the unmerged path (the child process) wrote another proof than the CPU prover"
