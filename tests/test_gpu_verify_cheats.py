"""cstark_tx_verify against a prover that cheats (tests/cheating_prover.py): proofs whose commitments, openings and folds are all
consistent and that ONE algebraic check alone can reject -- the out-of-domain equation on an invalid trace, the DEEP value against the
layer-0 row, the low-degree test on a forged out-of-domain value, a layer's count -- alone and in mixed batches; chosen query positions
(0, N - 1, a repeated draw, two positions in one layer-0 row); proofs with two faults, where the verdict order decides; every verdict
of the table; and a batch that spans several staging chunks.  test_oracle_cheats.py shows on the CPU that the restated verifier gives
each crafted proof exactly its isolating verdict."""
import os
import re
import struct
import time

import numpy as np
import pytest

import cheating_prover as CP
from test_gpu_verify import backend, names, oracle_verdict, words_canonical  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = list(CP.CONFIGS)
SEEN = set()   # every verdict cstark_tx_verify returned in this module


def gpu(backend, proofs, r0, r1):
    got = names(backend.tx_verify(proofs, r0, r1))
    SEEN.update(got)
    return got


def expected(proof, r0, r1):
    """the restated verifier's verdict, or MALFORMED for a word >= p (which the restated verifier does not look for)"""
    return oracle_verdict(proof, r0, r1) if words_canonical(proof) else "MALFORMED"


@pytest.fixture(scope="module")
def w(oracle):
    return CP.witness()


# ---- one check at a time ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
def test_one_check_at_a_time(backend, w, cfg):
    r0, r1 = w.initial_roots[0], w.final_root
    cases = CP.isolating_cases(cfg)
    report = []
    for name, (proof, required, _) in cases.items():
        got, ref = gpu(backend, [proof], r0, r1)[0], oracle_verdict(proof, r0, r1)
        report.append((name, got, ref, required))
    print(cfg, report)
    for name, got, ref, required in report:
        assert got == ref == required, (cfg, name, got, ref, required)


def test_crafted_proofs_in_one_batch(backend, w):
    """every crafted proof of the three configurations in one call, an honest proof after every second one"""
    r0, r1 = w.initial_roots[0], w.final_root
    proofs, want = [], []
    crafted = [(cfg, name, proof, required) for cfg in CFGS for name, (proof, required, _) in CP.isolating_cases(cfg).items() if name != "honest"]
    order = np.random.default_rng(5).permutation(len(crafted))   # the three extension degrees interleaved
    for i, j in enumerate(order):
        cfg, name, proof, required = crafted[j]
        proofs.append(proof); want.append(required)
        if i % 2 == 1:
            proofs.append(CP.isolating_cases(cfg)["honest"][0]); want.append("OK")
    assert want.count("OK") >= 20
    assert gpu(backend, proofs, r0, r1) == want


# ---- position edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
def test_position_edges(backend, w, cfg):
    from oracle import verifier as V
    r0, r1 = w.initial_roots[0], w.final_root
    o = CP.CONFIGS[cfg]
    m = o[4] + 1
    rows = CP._domain(o) // o[5]
    for want, (proof, q) in CP.edge_cases(cfg).items():
        assert gpu(backend, [proof], r0, r1) == ["OK"], (cfg, want)
        L = CP.layout(proof)
        pos = CP.query_positions(proof, r0, r1)
        slot = V.fold_positions(pos, rows).index(pos[q] & (rows - 1))
        bads = [CP.flip_at(proof, L["trace_rows"] + 8 * CP.W * q + 8 * 17 + 1, 0x04),           # the rows opened at the edge position
                CP.flip_at(proof, L["trace_paths"] + 32 * L["log_N"] * q + 3, 0x20),
                CP.flip_at(proof, L["cons_rows"] + 8 * CP.CE * m * q + 8 * 2, 0x02),
                CP.flip_at(proof, L["cons_paths"] + 32 * L["log_N"] * q + 32 * (L["log_N"] - 1) + 9, 0x01),
                CP.flip_at(proof, L["layers"][0]["rows"] + L["layers"][0]["row_bytes"] * slot + 8 * 1 + 2, 0x10),
                CP.flip_at(proof, L["layers"][0]["paths"] + 32 * L["layers"][0]["depth"] * slot + 5, 0x40)]
        ref = [expected(b, r0, r1) for b in bads]
        assert "OK" not in ref
        assert gpu(backend, bads, r0, r1) == ref, (cfg, want, q)


# ---- LAYER_COUNT and what ranks around it -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
def test_layer_count_among_other_faults(backend, w, cfg):
    r0, r1 = w.initial_roots[0], w.final_root
    o = CP.CONFIGS[cfg]
    proof = CP.isolating_cases(cfg)["honest"][0]
    nl = CP.layout(proof)["n_layers"]
    assert nl >= 2
    cases = []
    # a word >= p in a later layer: the rows after the mismatch have no positions to be opened at, but are still read
    cases.append(("noncanonical-later", CP.noncanonical(CP.layer_count(proof, 0, -1), "layer%d" % (nl - 1), 3), "MALFORMED"))
    # the DEEP values disagree with layer 0, and the last layer's count is wrong: the earlier check wins
    deep = CP.isolating_cases(cfg)["shifted_deep:component-0"][0]
    cases.append(("deep-then-count", CP.layer_count(deep, nl - 1, -1), "LAYER_FOLDING"))
    # layer 1 disagrees with the fold of layer 0: before a wrong count of layer 1 nothing, after a wrong count of layer 0 never reached
    fold = CP.perturbed_fold(w, o, 0)
    cases.append(("count-then-fold", CP.layer_count(fold, 0, -1), "LAYER_COUNT"))
    cases.append(("count-and-fold-same-layer", CP.layer_count(fold, 1, -1), "LAYER_COUNT"))
    if nl >= 3:
        cases.append(("fold-then-count", CP.layer_count(fold, 2, -1), "LAYER_FOLDING"))
    # a wrong count and a remainder that is not of low degree
    forged = CP.isolating_cases(cfg)["forged_ood:value"][0]
    cases.append(("count-then-degree", CP.layer_count(forged, nl - 1, -1), "LAYER_COUNT"))
    for name, p, required in cases:
        assert expected(p, r0, r1) == required, (cfg, name)
    assert gpu(backend, [p for _, p, _ in cases], r0, r1) == [r for _, _, r in cases]
    assert [gpu(backend, [p], r0, r1)[0] for _, p, _ in cases] == [r for _, _, r in cases]


# ---- two faults: the order decides ---------------------------------------------------------------------------------------------------
# grinding > 0 so that a changed nonce is a fault of its own
ORDER_CONFIGS = {"base-blake3": (8, 8, 4, 0, 0, 4, 128), "quadratic-sha3": (12, 8, 3, 1, 1, 8, 128), "cubic-blake3": (16, 8, 3, 0, 2, 16, 256)}


def _mutators(proof, r0, r1):
    """name -> (stage, function): single faults on disjoint bytes.  Stage 0 changes bytes in place, before the row and path that the
    stage 1 surgery on layer 0 removes (its last), so the offsets of the original proof hold for every pair."""
    from test_gpu_verify import _tamper_offsets
    L, T = CP.layout(proof), _tamper_offsets(proof)
    nq, m, log_N = L["nq"], L["m"], L["log_N"]
    R = L["rem_len"]
    queried = {p & (R - 1) for p in CP.query_positions(proof, r0, r1)}
    rem_q = min(queried)
    rem_u = min(set(range(R)) - queried - {rem_q + 1, 5})
    last = L["layers"][-1]
    at = {
        "ood": T["ood_comp"], "rem_commit": T["rem_commit"], "nonce": T["nonce"],
        "trace_row_first": L["trace_rows"] + 8 * 40, "trace_row_last": L["trace_rows"] + 8 * CP.W * (nq - 1) + 8 * 7,
        "cons_row_first": L["cons_rows"] + 8 * 1, "cons_row_last": L["cons_rows"] + 8 * CP.CE * m * (nq - 1) + 8 * 4,
        "layer0_row": L["layers"][0]["rows"] + 8 * 2, "last_layer_row": last["rows"] + 8 * 1,
        "remainder_queried": L["remainder"] + 8 * rem_q, "remainder_unqueried": L["remainder"] + 8 * rem_u,
    }
    assert len(set(o // 8 for o in at.values())) == len(at)
    assert L["n_layers"] == 1 or L["layers"][0]["npos"] >= 2
    muts = {name: (0, (lambda p, off=off: CP.flip_at(p, off, 0x01))) for name, off in at.items()}
    muts["remainder_noncanonical"] = (0, lambda p: CP.noncanonical(p, "remainder", 5 if rem_q != 5 else 6))
    muts["layer0_count"] = (1, lambda p: CP.layer_count(p, 0, -1))
    return muts


@pytest.mark.parametrize("cfg", list(ORDER_CONFIGS))
def test_first_failing_check_wins(backend, w, cfg):
    r0, r1 = w.initial_roots[0], w.final_root
    proof = CP.honest(w, ORDER_CONFIGS[cfg])
    muts = _mutators(proof, r0, r1)
    assert len(muts) == 13
    keys = list(muts)
    single = {k: muts[k][1](proof) for k in keys}
    single_ref = {k: expected(single[k], r0, r1) for k in keys}
    assert "OK" not in single_ref.values(), single_ref
    pairs, proofs = [], []
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            x, y = sorted((a, b), key=lambda k: muts[k][0])
            pairs.append((a, b))
            proofs.append(muts[y][1](muts[x][1](proof)))
    assert len(pairs) == 78
    ref = [expected(p, r0, r1) for p in proofs]
    decisive = sum(single_ref[a] != single_ref[b] for a, b in pairs)
    print(cfg, "single faults:", single_ref, "decisive pairs:", decisive)
    assert decisive >= 30
    # the pair's verdict is the earlier of its faults' verdicts in the order of include/cstark.h (a changed nonce also moves the
    # positions, so only the restated verifier says what a pair with it gives)
    from certificate_stark_amd import VERDICTS
    for (a, b), r in zip(pairs, ref):
        if "nonce" not in (a, b) and not {single_ref[a], single_ref[b]} == {"TRACE_OPENING", "COMPOSITION_OPENING"}:  # those: per query
            assert r == min(single_ref[a], single_ref[b], key=VERDICTS.index), (a, b, r)
    got_single = gpu(backend, [single[k] for k in keys], r0, r1)
    assert got_single == [single_ref[k] for k in keys]
    got = gpu(backend, proofs, r0, r1)
    for pair, g, r in zip(pairs, got, ref):
        assert g == r, (cfg, pair, g, r)


# ---- more than one chunk ------------------------------------------------------------------------------------------------------------
def chunk_bytes():
    hdr = open(os.path.join(ROOT, "include", "cstark.h")).read()
    return int(re.search(r"#define\s+CSTARK_VERIFY_CHUNK_BYTES\s+(\d+)", hdr).group(1))


def test_batch_of_several_chunks(backend, oracle, w):
    from oracle import prover as OP
    C = chunk_bytes()
    assert C == 64 << 20
    w2 = CP.witness(2, 3)
    big = CP.honest(w2, (128, 16, 0, 0, 2, 4, 128))
    count = int(2.5 * C / len(big)) + 1
    assert count * len(big) > 2.5 * C
    last_path = "layer%d_path" % (CP.layout(big)["n_layers"] - 1)
    small = CP.isolating_cases("cubic-blake3")
    # (proof, witness): mutations of the large proof, a crafted proof of another size and statement, another AIR's proof
    rejects = [(CP.flip(big, "remainder"), w2), (CP.flip(big, "ood_next"), w2), (CP.flip(big, "trace_row"), w2),
               (CP.noncanonical(big, "remainder", 9), w2), (CP.layer_count(big, 0, -1), w2), (CP.flip(big, last_path), w2),
               (small["forged_ood:value"][0], w), (small["shifted_deep:component-2"][0], w), (CP.flip(big, "cons_path"), w2)]
    merkle = (OP.prove_air(oracle.AIR_MERKLE, w2, (8, 8, 0, 0, 0, 4, 128)), w2)
    one = lambda p, ww: gpu(backend, [p], ww.initial_roots[0], ww.final_root)[0]
    t0 = time.perf_counter()
    assert one(big, w2) == "OK"
    single = [one(p, ww) for p, ww in rejects]
    assert single == ["REMAINDER_COMMITMENT", "OOD", "TRACE_OPENING", "MALFORMED", "LAYER_COUNT", "LAYER_OPENING", "REMAINDER_DEGREE",
                      "LAYER_FOLDING", "COMPOSITION_OPENING"]
    assert one(*merkle) == "UNSUPPORTED"
    # rejects at both ends, around every multiple of the budget counted in proof bytes (a chunk also holds its proofs' descriptors and
    # opening records, so it ends some proofs earlier: every 5th entry is a reject as well, which puts one within two entries of any
    # boundary), another AIR's proof -- which is not staged, so staged and caller indices differ from there on -- before the first
    at = {0, count - 1} | {int(k * C / len(big)) + d for k in range(1, int(count * len(big) / C) + 1) for d in (-1, 0, 1)}
    at |= set(range(0, count, 5))
    at = sorted(i for i in at if 0 <= i < count and i != 3)
    items, want = [(big, w2)] * count, ["OK"] * count
    for j, i in enumerate(at):
        items[i], want[i] = rejects[j % len(rejects)], single[j % len(rejects)]
    items[3], want[3] = merkle, "UNSUPPORTED"
    proofs = [p for p, _ in items]
    r0s = np.stack([ww.initial_roots[0] for _, ww in items])
    r1s = np.stack([ww.final_root for _, ww in items])
    t1 = time.perf_counter()
    got = gpu(backend, proofs, r0s, r1s)
    t2 = time.perf_counter()
    h2d, ms = backend.verify_h2d_bytes(), backend.verify_stage_ms()
    print("chunk test: %d proofs of %d bytes, %.1f MiB copied = at least %d chunks, singles %.2f s, batch %.2f s, stages %s"
          % (count, len(big), h2d / 2**20, -(-h2d // C), t1 - t0, t2 - t1, ms))
    assert got == want
    assert h2d > 2 * C          # one chunk never copies more than C: at least three ran
    assert len(ms) == 7 and all(v >= 0 for v in ms.values())
    # a small call after a large one, the large one again (arenas already grown, result slots hold the previous call's ranks)
    three = ([rejects[6][0], small["honest"][0], rejects[7][0]], w.initial_roots[0], w.final_root)
    want3 = ["REMAINDER_DEGREE", "OK", "LAYER_FOLDING"]
    assert gpu(backend, *three) == want3
    assert backend.verify_h2d_bytes() < C
    assert gpu(backend, proofs, r0s, r1s) == want
    assert backend.verify_h2d_bytes() == h2d
    assert gpu(backend, *three) == want3


# ---- every verdict --------------------------------------------------------------------------------------------------------------------
def test_every_rejecting_verdict_was_produced():
    """the tests above made cstark_tx_verify return every verdict a TransactionAir proof can be rejected with (run alone, this fails)"""
    need = {"MALFORMED", "OOD", "REMAINDER_COMMITMENT", "POW", "TRACE_OPENING", "COMPOSITION_OPENING", "LAYER_COUNT", "LAYER_OPENING",
            "LAYER_FOLDING", "REMAINDER_FOLDING", "REMAINDER_DEGREE"}
    assert need <= SEEN, sorted(need - SEEN)
