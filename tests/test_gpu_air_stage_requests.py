"""The sub-AIR constraint stage as one request (csrc/ctx.h AirStageRequest, capi.hip air_stage): every malformed request is refused
with the status the C ABI has always given it, and a context that has refused them still evaluates -- RangeProofAir (64 rows) and
MerkleAir (1 transfer, depth 3, 512 rows) at blowup 8, materialised and fused, twice each with different coefficients so that the second
call runs on the cached per-AIR tables and the reused staging block -- bit-exact against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5
u64p = C.POINTER(C.c_uint64)
LOG_B = 3


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """per AIR: the extended trace, its transition values, and two coefficient sets with the oracle's merged evaluations (computed once)"""
    number = 0x0123456789ABCDEF
    w = oracle.TxWitness.generate(1, 3, seed=901)
    out = {}
    for name, trace, desc, ptab_cols, nc, na in (
            ("range", oracle.range_build_trace(number), oracle.range_desc(number), None, 2, 2),
            ("merkle", oracle.merkle_build_trace(w), None, oracle.merkle_periodic_columns(3), 106, 14)):
        if desc is None:
            desc = oracle.merkle_desc(trace)
        log_n = trace.shape[1].bit_length() - 1
        lde = oracle.lde_columns(oracle.interpolate_columns(trace), LOG_B)
        ptab = None if ptab_cols is None else oracle.periodic_table(ptab_cols, log_n, LOG_B)
        ev = oracle.air_evaluate_transitions(oracle.AIR_RANGE if name == "range" else oracle.AIR_MERKLE, lde, ptab, nc)
        sets = []
        for seed in (11, 29):
            cf = [oracle.random_elements(nc, seed), oracle.random_elements(nc, seed + 1), oracle.random_elements(na, seed + 2), oracle.random_elements(na, seed + 3)]
            sets.append((cf, oracle.air_combine(desc, lde, ev, *cf, LOG_B)))
        out[name] = dict(log_n=log_n, lde=lde, ev=ev, a_value=desc.a_value, sets=sets)
    assert out["range"]["log_n"] == 6 and out["merkle"]["log_n"] == 9
    return out


def _host(a):
    return None if a is None else np.ascontiguousarray(a, np.uint64)


def _hp(a):
    return None if a is None else a.ctypes.data_as(u64p)


def _dp(t):
    """device pointer of a tensor, or NULL"""
    return None if t is None else C.cast(C.c_void_p(t.data_ptr()), u64p)


def test_refused_requests_leave_a_working_context(oracle, backend, cases):
    from certificate_stark_amd.backend import to_numpy_u64
    lib, ctx = backend.lib, backend.ctx
    rg = cases["range"]
    d_lde, d_ev = backend.from_numpy_u64(rg["lde"]), backend.from_numpy_u64(rg["ev"])
    d_out = backend.empty_u64(8, 64)
    coefs = [_host(a) for a in rg["sets"][0][0]]
    avals = _host(rg["a_value"])
    wide = [_host(oracle.random_elements(106, 5)) for _ in range(4)]   # long enough for MerkleAir's 106 and SchnorrAir's 56 / 61
    # The refused 512-row MerkleAir and SchnorrAir requests are turned away before anything is launched; their tables are still sized
    # for the request (the largest is MerkleAir's [8][106][512] transition values), so a wrong status could never be an out-of-bounds read.
    big = torch.zeros((8, 106, 512), dtype=torch.int64, device=backend.device)
    big_out = backend.empty_u64(8, 512)

    def combine(air=backend.AIR_RANGE, n_items=0, lde=d_lde, evals=d_ev, cf=coefs, av=avals, avals_lde=None, n_avals=0, out=d_out, log_n=6, log_b=LOG_B, k0=0, nk=8):
        return lib.cstark_air_combine(ctx, C.c_int(air), C.c_uint32(n_items), _dp(lde), _dp(evals), *[_hp(a) for a in cf], _hp(av), _dp(avals_lde),
                                      C.c_uint32(n_avals), _dp(out), C.c_uint32(log_n), C.c_uint32(log_b), C.c_uint32(k0), C.c_uint32(nk))

    def merkle_fused(depth, log_b=LOG_B, nk=8):
        return lib.cstark_merkle_evaluate_constraints(ctx, C.c_uint32(depth), _dp(big), *[_hp(a) for a in wide], _hp(wide[0]), _dp(big_out), C.c_uint32(9),
                                                      C.c_uint32(log_b), C.c_uint32(0), C.c_uint32(nk))

    def schnorr_fused(aux):
        return lib.cstark_schnorr_evaluate_constraints(ctx, C.c_uint32(1), _dp(big), _dp(aux), *[_hp(a) for a in wide], _dp(big), C.c_uint32(12), _dp(big_out),
                                                       C.c_uint32(9), C.c_uint32(LOG_B), C.c_uint32(0), C.c_uint32(8))

    without = lambda i: coefs[:i] + [None] + coefs[i + 1:]
    refused = [
        ("null d_lde", lambda: combine(lde=None), INVALID_ARG),
        ("null d_out", lambda: combine(out=None), INVALID_ARG),
        ("null t_alpha", lambda: combine(cf=without(0)), INVALID_ARG),
        ("null t_beta", lambda: combine(cf=without(1)), INVALID_ARG),
        ("null b_alpha", lambda: combine(cf=without(2)), INVALID_ARG),
        ("null b_beta", lambda: combine(cf=without(3)), INVALID_ARG),
        ("nk = 0", lambda: combine(nk=0), INVALID_ARG),
        ("cstark_air_combine with null d_evals", lambda: combine(evals=None), INVALID_ARG),
        ("air id 0", lambda: combine(air=0), UNSUPPORTED),
        ("air id 5", lambda: combine(air=5), UNSUPPORTED),
        ("RangeProofAir without assertion values", lambda: combine(av=None), INVALID_ARG),
        ("SchnorrAir merge without d_avals_lde",
         lambda: combine(air=backend.AIR_SCHNORR, n_items=1, lde=big, evals=big, cf=wide, av=None, out=big_out, log_n=9), INVALID_ARG),
        ("MerkleAir at blowup 2, below its constraint degree",
         lambda: combine(air=backend.AIR_MERKLE, lde=big, evals=big, cf=wide, av=wide[0], out=big_out, log_n=9, log_b=1, nk=2), INVALID_ARG),
        ("MerkleAir fused at blowup 2", lambda: merkle_fused(3, log_b=1, nk=2), INVALID_ARG),
        ("k0 + nk beyond the blowup", lambda: combine(k0=4), INVALID_ARG),
        ("log_blowup = 4", lambda: combine(log_b=4), UNSUPPORTED),
        ("cstark_merkle_evaluate_constraints with depth 32", lambda: merkle_fused(32), INVALID_ARG),
        ("cstark_schnorr_evaluate_constraints with null d_aux_lde", lambda: schnorr_fused(None), INVALID_ARG),
    ]
    for name, call, status in refused:
        assert call() == status, name
        assert lib.cstark_last_error(), name

    # the same context: both AIRs, materialised and fused, two coefficient sets each (the second on the cached tables)
    mk = cases["merkle"]
    d_mlde = backend.from_numpy_u64(mk["lde"])
    d_rev = backend.air_evaluate_transitions(backend.AIR_RANGE, d_lde, 0, LOG_B)
    d_mev = backend.air_evaluate_transitions(backend.AIR_MERKLE, d_mlde, 3, LOG_B)
    assert (to_numpy_u64(d_rev) == rg["ev"]).all() and (to_numpy_u64(d_mev) == mk["ev"]).all()
    for cf, ref in rg["sets"]:
        got = backend.air_combine(backend.AIR_RANGE, d_lde, d_rev, *cf, rg["a_value"], LOG_B)
        assert (to_numpy_u64(got) == ref).all()
    for cf, ref in mk["sets"]:
        got = backend.air_combine(backend.AIR_MERKLE, d_mlde, d_mev, *cf, mk["a_value"], LOG_B)
        assert (to_numpy_u64(got) == ref).all()
        fused = backend.merkle_evaluate_constraints(d_mlde, 3, *cf, mk["a_value"], LOG_B)
        assert (to_numpy_u64(fused) == ref).all()
    assert not np.array_equal(mk["sets"][0][1], mk["sets"][1][1]) and not np.array_equal(rg["sets"][0][1], rg["sets"][1][1])
