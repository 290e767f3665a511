"""The proofs of tests/cheating_prover.py against the restated verifier (oracle/verifier.py), on the CPU: each must be rejected by
exactly the one check it was built for -- the guarantee that test_gpu_verify_cheats.py, which runs the same proofs through
cstark_tx_verify, is not vacuous.  No case is skipped for giving another verdict."""
import pytest

import cheating_prover as CP
from test_gpu_verify import oracle_verdict

CFGS = list(CP.CONFIGS)


def _message(proof, w):
    from oracle import verifier as V
    try:
        V.verify(proof, w.initial_roots[0], w.final_root)
        return ""
    except V.VerifierError as e:
        return str(e)


@pytest.mark.parametrize("builder", ["invalid_trace", "wrong_composition", "shifted_deep", "forged_ood", "layer_count", "perturbed_fold"])
@pytest.mark.parametrize("cfg", CFGS)
def test_each_cheat_fails_one_check_only(oracle, cfg, builder):
    w = CP.witness()
    cases = {k: v for k, v in CP.isolating_cases(cfg).items() if k.startswith(builder)}
    assert len(cases) >= (5 if builder == "invalid_trace" else 2 if builder != "shifted_deep" else CP.CONFIGS[cfg][4] + 1)
    for name, (proof, verdict, part) in cases.items():
        assert oracle_verdict(proof, w.initial_roots[0], w.final_root, options=list(CP.CONFIGS[cfg])) == verdict, (cfg, name)
        assert part in _message(proof, w), (cfg, name)


def test_a_layer_count_case_grows(oracle):
    """delta = +1 needs a layer with fewer rows than queries: at least one configuration has one"""
    assert any(k.endswith("+1") for cfg in CFGS for k in CP.isolating_cases(cfg))


@pytest.mark.parametrize("cfg", CFGS)
def test_honest_proof_and_chosen_positions_are_accepted(oracle, cfg):
    w = CP.witness()
    r0, r1 = w.initial_roots[0], w.final_root
    o = CP.CONFIGS[cfg]
    N, rows = CP._domain(o), CP._domain(o) // o[5]
    assert oracle_verdict(CP.isolating_cases(cfg)["honest"][0], r0, r1, options=list(o)) == "OK"
    for want, (proof, q) in CP.edge_cases(cfg).items():
        assert oracle_verdict(proof, r0, r1, options=list(o)) == "OK", (cfg, want)
        pos, draws = CP.query_replay(proof, r0, r1)
        assert len(set(pos)) == o[0]
        if want == "first":
            assert pos[q] == 0
        elif want == "last":
            assert pos[q] == N - 1
        elif want == "repeat":   # the coin produced pos[q] twice and the second one was skipped
            assert len(draws) > o[0] and draws.count(pos[q]) >= 2
        elif want == "same-row":
            assert pos[q] & (rows - 1) in [p & (rows - 1) for p in pos[:q]]


def test_default_nonce_is_one(oracle):
    """without the hook and without proof of work the prover writes nonce 1, as before (the bytes of default proofs as a whole are
    pinned by the golden digests of the existing oracle tests)"""
    import struct
    proof = CP.isolating_cases(CFGS[0])["honest"][0]
    assert struct.unpack_from("<Q", proof, CP.layout(proof)["nonce"])[0] == 1


def test_byte_surgery_parses(oracle):
    from certificate_stark_amd import inspect_proof
    for cfg in CFGS:
        for name, (proof, _, _) in CP.isolating_cases(cfg).items():
            if name.startswith("layer_count"):
                assert inspect_proof(proof).verdict == 0, (cfg, name)
