"""cstark_air_verify on the GPU: MerkleAir, RangeProofAir and RescueAir proofs through the pipeline of cstark_tx_verify.  The
reference's sub-AIR acceptance tests with the product verifier, every section tampered with against the restated verifier
(oracle/verifier.py: verify_merkle / verify_range / verify_rescue), the cheating prover of cheating_sub_airs.py, mixed batches, misuse.
SchnorrAir has no verifier: its proofs are UNSUPPORTED through both calls."""
import ctypes as C
import struct

import numpy as np
import pytest

import cheating_sub_airs as CS
from test_gpu_verify import example, names, oracle_verdict as tx_oracle_verdict

pytestmark = pytest.mark.gpu
P = CS.P


def _opts(t):
    from certificate_stark_amd.prover import ProofOptions
    return ProofOptions(*t)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def oracle_verdict(air, proof, pub, options=None):
    """The restated verifier's reason for a proof stated to be of `air`, through the message table of test_gpu_verify.oracle_verdict:
    that function asks oracle.verifier.verify, which stands for the sub-AIR's entry point while it runs."""
    from oracle import verifier as Vf
    pub = np.asarray(pub, np.uint64)
    if air == 0:
        return tx_oracle_verdict(proof, pub[:7], pub[7:], options)
    real = Vf.verify
    Vf.verify = lambda proof, r0, r1, options=None: CS.verify(air, proof, np.concatenate([r0, r1]), options=options)
    try:
        return tx_oracle_verdict(proof, pub[:7], pub[7:], options)
    finally:
        Vf.verify = real


def expected(air, proof, pub, options=None):
    return oracle_verdict(air, proof, pub, options) if CS.words_canonical(proof) else "MALFORMED"


def air_verify(backend, items, options=None):
    """items: (AIR, proof, 14 public words)"""
    return names(backend.air_verify([p for _, p, _ in items], [a for a, _, _ in items], np.stack([np.asarray(w, np.uint64) for _, _, w in items]),
                                    options))


# ---- 1. acceptance: the GPU provers' proofs ---------------------------------------------------------------------------------------------
def _merkle_example(backend, n_tx, depth, o, seed=0x5EED):
    from oracle import oracle as O
    from certificate_stark_amd.prover import MerkleExample, TransactionMetadata
    w = O.TxWitness.generate(n_tx, depth, seed=seed)
    return MerkleExample(_opts(o), TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS]), backend)


def _wrong_words(pub, words):
    for k in words:
        bad = np.array(pub, np.uint64, copy=True)
        bad[k] = (int(bad[k]) + 1) % P
        yield bad


# ce = 4 below the blowup at 8; every extension degree, both hashes, every folding factor, proof of work
MERKLE_CASES = [(1, 3, (8, 4, 0, 0, 0, 4, 128)), (2, 7, (12, 8, 0, 1, 1, 8, 256)), (1, 3, (16, 8, 3, 0, 2, 16, 128)), (2, 7, (8, 4, 0, 1, 0, 4, 1024))]


def test_merkle_proof_verification(backend):
    """src/merkle/update/tests.rs: the proof verifies; with wrong public inputs (every one of the 14 words) it does not.  The two
    depth-7 proofs and the two depth-3 proofs of one call use two periodic tables."""
    from certificate_stark_amd import VerifierError
    items = []
    for n_tx, depth, o in MERKLE_CASES:
        ex = _merkle_example(backend, n_tx, depth, o)
        proof = ex.prove()
        ex.verify(proof)
        pub = np.concatenate(ex.pub_inputs())
        assert CS.verify(CS.MERKLE, proof, pub, options=list(o))
        items.append((CS.MERKLE, proof, pub))
    assert air_verify(backend, items) == ["OK"] * len(items)
    air, proof, pub = items[0]
    assert air_verify(backend, [(air, proof, bad) for bad in _wrong_words(pub, range(14))]) == ["OOD"] * 14
    ex.tx_metadata.final_root = np.array(ex.tx_metadata.final_root[::-1], np.uint64)
    with pytest.raises(VerifierError) as e:
        ex.verify(items[-1][1])
    assert e.value.reason == "OOD"


# 64 rows: no FRI layer (the remainder is the whole DEEP evaluation) and one layer
RANGE_CASES = [(8, 2, 0, 0, 1, 4, 128), (8, 4, 0, 0, 0, 4, 256), (8, 4, 0, 0, 0, 4, 128), (8, 8, 0, 1, 2, 8, 128), (12, 8, 2, 1, 0, 16, 128)]


def test_range_proof_verification(backend):
    """src/range/tests.rs: the reference's 64-row proof at every shape of its FRI, the long form, and one proof of a batched call"""
    from oracle import oracle as O
    from certificate_stark_amd import VerifierError
    from certificate_stark_amd.prover import RangeProofExample
    number = CS.mont(CS.NUMBER)
    items = []
    for o in RANGE_CASES:
        ex = RangeProofExample(_opts(o), number, backend)
        proof = ex.prove()
        assert CS.layout(proof)["n_layers"] == (0 if 64 * o[1] <= o[6] else 1)
        ex.verify(proof)
        assert CS.verify(CS.RANGE, proof, [number], options=list(o))
        items.append((CS.RANGE, proof, np.array([number] + [0] * 13, np.uint64)))
    words = np.random.default_rng(3).integers(0, 2**63, size=16, dtype=np.uint64)   # 2^10 rows
    o = (10, 8, 0, 0, 1, 4, 256)
    long_number = O.range_build_trace_bits(words, 10)[1]
    items.append((CS.RANGE, backend.range_prove_bits(_opts(o), words, 10), np.array([long_number] + [0] * 13, np.uint64)))
    numbers = O.to_mont(np.array([0, 17, 2**63 - 1, P - 1], np.uint64))
    batch = backend.range_prove_batch(_opts((8, 8, 0, 0, 0, 4, 128)), numbers)
    items.append((CS.RANGE, batch[2], np.array([numbers[2]] + [P - 1] * 13, np.uint64)))   # words 1..13 are ignored
    assert air_verify(backend, items) == ["OK"] * len(items)
    assert names(backend.air_verify(list(batch), CS.RANGE, numbers=numbers)) == ["OK"] * 4
    fourteen = O.to_mont(np.arange(100, 114, dtype=np.uint64))      # [count] numbers with count = 14 are numbers, not one statement
    assert names(backend.air_verify(list(backend.range_prove_batch(_opts((8, 8, 0, 0, 0, 4, 128)), fourteen)), CS.RANGE, numbers=fourteen)) == ["OK"] * 14
    with pytest.raises(ValueError):
        backend.air_verify(list(batch), [CS.RANGE, CS.RANGE, CS.MERKLE, CS.RANGE], numbers=numbers)
    assert air_verify(backend, [(a, p, next(_wrong_words(w, [0]))) for a, p, w in items]) == ["OOD"] * len(items)
    with pytest.raises(VerifierError) as e:
        RangeProofExample(_opts(RANGE_CASES[0]), CS.mont(CS.NUMBER + 1), backend).verify(items[0][1])
    assert e.value.reason == "OOD"


RESCUE_CASES = [(8, (8, 4, 0, 0, 0, 4, 128)), (8, (10, 4, 0, 1, 1, 8, 128)), (16, (8, 8, 0, 0, 2, 16, 256))]


def test_rescue_proof_verification(backend):
    """benches/rescue.rs:88-94"""
    from certificate_stark_amd import VerifierError
    from certificate_stark_amd.prover import RescueExample
    items = []
    for chain, o in RESCUE_CASES:
        ex = RescueExample(chain, _opts(o), backend)
        proof = ex.prove()
        ex.verify(proof)
        pub = np.concatenate(ex.pub_inputs())
        assert CS.verify(CS.RESCUE, proof, pub, options=list(o))
        items.append((CS.RESCUE, proof, pub))
    assert air_verify(backend, items) == ["OK"] * len(items)
    air, proof, pub = items[0]
    assert air_verify(backend, [(air, proof, bad) for bad in _wrong_words(pub, range(14))]) == ["OOD"] * 14
    other = RescueExample(8, _opts(RESCUE_CASES[0][1]), backend, seed=pub[7:])
    with pytest.raises(VerifierError):
        other.verify(proof)


# ---- 2. against the restated verifier -----------------------------------------------------------------------------------------------------
def _tamper_options(air, ext):
    nq, blowup, _, _, _, fold, rem = CS.OPTIONS[air]
    return (nq, 8, 0, ext % 2, ext, (4, 8, 16)[ext], rem)   # at least one FRI layer for every AIR


@pytest.mark.parametrize("ext", [0, 1, 2])
@pytest.mark.parametrize("air", [CS.MERKLE, CS.RANGE, CS.RESCUE])
def test_tampered_sections(backend, air, ext):
    """one bit flipped in every section, a word >= p in every element section, a truncated proof, other expected options"""
    o = _tamper_options(air, ext)
    proof, pub = CS.honest(air, o)
    assert CS.layout(proof)["n_layers"] >= 1 and CS.layout(proof)["m"] == ext + 1
    cases = [("honest", proof)]
    for name, off in CS.tamper_offsets(proof).items():
        bad = bytearray(proof)
        bad[off] ^= 0x04
        cases.append((name, bytes(bad)))
    for sec in CS.element_sections(proof):
        cases.append((sec + ">=p", CS.noncanonical(proof, sec)))
    cases.append(("truncated", proof[:-8]))
    cases.append(("truncated-in-header", proof[:100]))
    expect = [expected(air, p, pub) for _, p in cases]
    got = air_verify(backend, [(air, p, pub) for _, p in cases])
    for (name, _), g, e in zip(cases, got, expect):
        assert g == e and (g != "OK") == (name != "honest"), (name, g, e)
    assert {"MALFORMED", "OOD", "TRACE_OPENING", "COMPOSITION_OPENING", "LAYER_OPENING", "REMAINDER_COMMITMENT"} <= set(got)
    for field in range(7):
        e = list(o)
        e[field] = e[field] + 1 if field != 1 else 16
        assert air_verify(backend, [(air, proof, pub)], _opts(tuple(e))) == ["OPTIONS_MISMATCH"] == [oracle_verdict(air, proof, pub, e)], field
    assert air_verify(backend, [(air, proof, pub)], _opts(o)) == ["OK"]


def test_tampered_proof_without_a_fri_layer(backend):
    o = (8, 4, 0, 0, 1, 4, 256)
    proof, pub = CS.honest(CS.RANGE, o)
    assert CS.layout(proof)["n_layers"] == 0
    cases = [("honest", proof)]
    for name, off in CS.tamper_offsets(proof).items():
        bad = bytearray(proof)
        bad[off] ^= 0x04
        cases.append((name, bytes(bad)))
    got = air_verify(backend, [(CS.RANGE, p, pub) for _, p in cases])
    for (name, p), g in zip(cases, got):
        assert g == expected(CS.RANGE, p, pub), name
    assert "REMAINDER_COMMITMENT" in got and got[0] == "OK" and got.count("OK") == 1   # (REMAINDER_FOLDING without a layer: the shifted DEEP cheat)


def test_header_values_no_prover_writes(backend):
    """a Merkle depth the witness upload refuses, a chain length that is not the trace's, a range header word: MALFORMED, while
    cstark_proof_inspect's answer does not change"""
    from certificate_stark_amd import inspect_proof
    cases = []
    for air, words in ((CS.MERKLE, (4, 0, 64)), (CS.RESCUE, (16, 0)), (CS.RANGE, (1,))):
        proof, pub = CS.honest(air, CS.OPTIONS[air])
        for w in words:
            bad = bytearray(proof)
            struct.pack_into("<I", bad, 20, w)
            assert inspect_proof(bytes(bad)).verdict == 0
            cases.append((air, bytes(bad), pub))
    assert air_verify(backend, cases) == ["MALFORMED"] * len(cases)
    proof, pub = CS.honest(CS.MERKLE, CS.OPTIONS[CS.MERKLE])
    bad = bytearray(proof)
    struct.pack_into("<I", bad, 20, 7)        # another depth the prover accepts: another periodic table, so the equation fails
    assert air_verify(backend, [(CS.MERKLE, bytes(bad), pub)]) == ["OOD"]


# ---- 3. the cheating prover ---------------------------------------------------------------------------------------------------------------
def test_cheating_prover_is_caught_by_the_isolating_check(backend):
    cases = CS.isolating_cases()
    # the control: the same prover without a deviation is accepted, so a rejection below is the deviation's
    assert air_verify(backend, [(air, *CS.honest(air, CS.OPTIONS[air])) for air in (CS.MERKLE, CS.RANGE, CS.RESCUE)]) == ["OK"] * 3
    got = air_verify(backend, [(air, proof, pub) for air, proof, pub, _, _ in cases.values()])
    for (name, (air, proof, pub, verdict, _)), g in zip(cases.items(), got):
        assert g == verdict == oracle_verdict(air, proof, pub), (name, g)


# ---- 4. one call, everything ----------------------------------------------------------------------------------------------------------------
def test_mixed_batch_in_one_call(backend, oracle):
    from oracle import prover as OP
    cases = CS.isolating_cases()
    items = []
    for ext, air in ((0, CS.MERKLE), (1, CS.RANGE), (2, CS.RESCUE), (2, CS.MERKLE), (0, CS.RANGE), (1, CS.RESCUE)):
        items.append((air, *CS.honest(air, _tamper_options(air, ext))))
        cheat = "lying_statement:" + CS.NAMES[air] if ext else "invalid_trace:%s:%d,%d" % ((CS.NAMES[air],) + CS.CELLS[air][0])
        items.append(cases[cheat][:3])
    items.append(cases["shifted_deep:no-layer"][:3])
    items.append((CS.RANGE, *CS.honest(CS.RANGE, (8, 2, 0, 1, 2, 4, 128))))
    tx = [example(1, 3, (8, 8, 0, 0, 0, 4, 128), backend=backend), example(2, 3, (12, 8, 0, 1, 2, 8, 256), seed=7, backend=backend)]
    tx_items = []
    for t in tx:
        proof, pub = t.prove(), np.concatenate(t.pub_inputs())
        bad = bytearray(proof)
        bad[len(proof) - 20] ^= 0x10
        tx_items += [(0, proof, pub), (0, bytes(bad), pub), (0, proof, pub[::-1].copy())]
    items[3:3] = tx_items[:3]
    items += tx_items[3:]
    sw = oracle.SchnorrWitness.generate(1, seed=9)
    schnorr = OP.prove_air(oracle.AIR_SCHNORR, sw, (8, 8, 0, 0, 0, 4, 128))
    merkle, merkle_pub = CS.honest(CS.MERKLE, CS.OPTIONS[CS.MERKLE])
    unsupported = [len(items), len(items) + 1, len(items) + 2]
    items += [(CS.SCHNORR, schnorr, np.zeros(14, np.uint64)), (CS.RANGE, merkle, merkle_pub), (CS.MERKLE, schnorr, merkle_pub)]
    items.insert(1, (CS.SCHNORR, CS.noncanonical(schnorr, "trace_rows"), np.full(14, P, np.uint64)))   # scanned first; its statement is not read
    unsupported = [i + 1 for i in unsupported]

    batch = air_verify(backend, items)
    single = [air_verify(backend, [it])[0] for it in items]
    assert batch == single
    assert [batch[i] for i in unsupported] == ["UNSUPPORTED"] * 3 and batch[1] == "MALFORMED"
    order = np.random.default_rng(11).permutation(len(items))
    assert [air_verify(backend, [items[i] for i in order])[k] for k in np.argsort(order)] == batch
    for i, (air, proof, pub) in enumerate(items):
        if i in unsupported or i == 1:
            continue
        assert batch[i] == expected(air, proof, pub), i
        if air == 0:
            assert batch[i] == names(backend.tx_verify([proof], pub[:7], pub[7:]))[0], i
    assert batch.count("OK") == 6 + 1 + 2 and {"OOD", "REMAINDER_FOLDING", "REMAINDER_COMMITMENT"} <= set(batch)
    # sub-AIR and SchnorrAir proofs through the TransactionAir call: as before
    assert names(backend.tx_verify([merkle, schnorr, items[0][1]], merkle_pub[:7], merkle_pub[7:])) == ["UNSUPPORTED"] * 3


def test_stage_times_and_copied_bytes_are_those_of_the_last_call(backend):
    proof, pub = CS.honest(CS.RANGE, CS.OPTIONS[CS.RANGE])
    assert air_verify(backend, [(CS.RANGE, proof, pub)] * 3) == ["OK"] * 3
    three, ms = backend.verify_h2d_bytes(), backend.verify_stage_ms()
    assert 3 * len(proof) < three < 3 * len(proof) + 65536 and all(v >= 0 for v in ms.values()) and ms["ood"] > 0
    assert air_verify(backend, [(CS.RANGE, proof, pub)]) == ["OK"]
    assert len(proof) < backend.verify_h2d_bytes() < three


# ---- 5. misuse ------------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_a_status_not_a_verdict(backend):
    from certificate_stark_amd._lib import CstarkError
    proof, pub = CS.honest(CS.RESCUE, CS.OPTIONS[CS.RESCUE])
    lib, ctx = backend.lib, backend.ctx
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    ptrs = (C.POINTER(C.c_uint8) * 1)(C.cast(buf, C.POINTER(C.c_uint8)))
    lens = (C.c_size_t * 1)(len(proof))
    airs = (C.c_int32 * 1)(CS.RESCUE)
    words = (C.c_uint64 * 14)(*[int(v) for v in pub])
    verdict = (C.c_int32 * 1)(-7)
    assert lib.cstark_air_verify(ctx, C.c_uint32(1), ptrs, lens, airs, words, None, verdict) == 0 and verdict[0] == 0
    for args in ((None, lens, airs, words, None, verdict), (ptrs, None, airs, words, None, verdict), (ptrs, lens, None, words, None, verdict),
                 (ptrs, lens, airs, None, None, verdict), (ptrs, lens, airs, words, None, None)):
        assert lib.cstark_air_verify(ctx, C.c_uint32(1), *args) < 0
    assert lib.cstark_air_verify(None, C.c_uint32(1), ptrs, lens, airs, words, None, verdict) < 0
    assert lib.cstark_air_verify(ctx, C.c_uint32(0), None, None, None, None, None, None) == 0
    for bad_air in (5, -1, 1 << 20):
        with pytest.raises(CstarkError):
            backend.air_verify([proof], bad_air, pub)
    for k in range(14):
        bad = np.array(pub, np.uint64, copy=True)
        bad[k] = P
        with pytest.raises(CstarkError):
            backend.air_verify([proof], CS.RESCUE, bad)
    with pytest.raises(CstarkError):
        backend.air_verify([proof], CS.RANGE, np.array([P] + [0] * 13, np.uint64))
    assert names(backend.air_verify([proof], CS.RANGE, np.array([0] + [P] * 13, np.uint64))) == ["UNSUPPORTED"]   # unused words are not read
    assert names(backend.air_verify([b"", b"CSTK", proof[:51]], CS.RESCUE, pub)) == ["MALFORMED"] * 3


def test_context_that_has_never_proved(oracle):
    from certificate_stark_amd.backend import Backend
    fresh = Backend()
    try:
        items = [(air, *CS.honest(air, CS.OPTIONS[air])) for air in (CS.RESCUE, CS.MERKLE, CS.RANGE)]
        assert air_verify(fresh, items) == ["OK"] * 3
    finally:
        fresh.close()
