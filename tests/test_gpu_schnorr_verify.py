"""cstark_schnorr_verify on the GPU: SchnorrAir proofs against their O(n) statement through the pipeline of cstark_air_verify.  The
reference's acceptance test (src/schnorr/tests.rs) with the product verifier, every word of a statement changed, every section of a proof
tampered with against the restated verifier (oracle/verifier.py, verify_schnorr), the cheating prover of cheating_schnorr.py, proofs of
another AIR, a batch of two chunks, misuse."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import cheating_schnorr as CS
import cheating_sub_airs as CSA
from test_gpu_verify import names

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


def statement_of(ex):
    """an example's statement as the restated verifier takes it"""
    from oracle import oracle as O
    w = O.SchnorrWitness(ex.messages.shape[0])
    w.messages, w.sig_rx, w.sig_s = np.array(ex.messages), np.array(ex.sig_rx), np.array(ex.sig_s)
    return w


def schnorr_verify(backend, items, options=None):
    """items: (proof, statement)"""
    return names(backend.schnorr_verify([p for p, _ in items], [w for _, w in items], options))


def expected(proof, w, options=None):
    return CS.oracle_verdict(proof, w, options) if CSA.words_canonical(proof) else "MALFORMED"


# ---- 1. acceptance ----------------------------------------------------------------------------------------------------------------------
# every extension degree, both hashes, every folding factor, proof of work, blowup above the constraint-evaluation blowup
CASES = [(1, (8, 8, 0, 0, 0, 4, 128)), (2, (12, 8, 0, 1, 1, 8, 256)), (1, (16, 8, 3, 0, 2, 16, 128)), (4, (8, 16, 0, 1, 0, 4, 1024))]


def test_schnorr_proof_verification(backend, oracle):
    """src/schnorr/tests.rs: the GPU prover's proofs verify -- through the example, in one batched call, and by the restated verifier"""
    from oracle import verifier as V
    from certificate_stark_amd.prover import SchnorrExample
    items = []
    for n_sig, o in CASES:
        ex = SchnorrExample.build_random(_opts(o), n_sig, seed=0x5EED + n_sig, backend=backend)
        proof = ex.prove()
        ex.verify(proof)
        w = statement_of(ex)
        assert V.verify_schnorr(proof, w, options=list(o))
        items.append((proof, w))
    assert schnorr_verify(backend, items) == ["OK"] * len(items)
    for (proof, w), (_, o) in zip(items, CASES):
        assert schnorr_verify(backend, [(proof, w)], _opts(o)) == ["OK"]
    # the existing calls still have no statement to verify it against
    assert names(backend.air_verify([items[0][0]], CSA.SCHNORR, np.zeros(14, np.uint64))) == ["UNSUPPORTED"]


def test_example_rejects_another_statement(backend, oracle):
    from certificate_stark_amd import VerifierError
    from certificate_stark_amd.prover import SchnorrExample
    proof, w = CS.honest()
    other = SchnorrExample.build_random(_opts(CS.OPTIONS), 1, seed=77, backend=backend)
    with pytest.raises(VerifierError) as e:
        other.verify(proof)
    assert e.value.reason == "OOD"
    SchnorrExample(_opts(CS.OPTIONS), w.messages, w.sig_rx, w.sig_s, backend).verify(proof)


# ---- 2. a wrong statement ---------------------------------------------------------------------------------------------------------------
def test_every_word_of_the_statement_is_bound(backend, oracle):
    """2 signatures: every one of the 34 words of the first and of the last signature + 1, one flipped s byte per signature, a statement
    with twice and with half as many signatures -- one call, all OOD, and the restated verifier rejects every one"""
    proof, w = CS.honest(2, CS.OPTIONS)
    wrong = []
    for t in (0, 1):
        wrong += [CS.changed(w, "messages", t, k) for k in range(28)] + [CS.changed(w, "sig_rx", t, k) for k in range(6)]
    wrong += [CS.changed(w, "sig_s", 0, 5), CS.changed(w, "sig_s", 1, 31)]
    wrong += [CS.witness(4), CS.witness(1)]
    three = CS.witness(4)
    three.n_sig, three.messages, three.sig_rx, three.sig_s = 3, three.messages[:3], three.sig_rx[:3], three.sig_s[:3]
    wrong.append(three)   # not a power of two
    got = schnorr_verify(backend, [(proof, w)] + [(proof, s) for s in wrong])
    assert got == ["OK"] + ["OOD"] * len(wrong)
    for s in wrong:
        assert CS.oracle_verdict(proof, s) == "OOD"
    # the count is decided after the layout, the AIR and the expected options
    other = tuple(list(CS.OPTIONS[:-1]) + [256])
    assert schnorr_verify(backend, [(proof, CS.witness(4))], _opts(other)) == ["OPTIONS_MISMATCH"]
    assert schnorr_verify(backend, [(CSA.noncanonical(proof, "trace_rows"), CS.witness(4)), (proof[:-8], CS.witness(4))]) == ["MALFORMED"] * 2


# ---- 3. against the restated verifier ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tampered(ext):
    o = (8, 8, 0, ext % 2, ext, (4, 8, 16)[ext], 128)
    proof, w = CS.honest(1, o)
    assert CSA.layout(proof)["n_layers"] >= 1 and CSA.layout(proof)["m"] == ext + 1
    cases = [("honest", proof)]
    for name, off in CSA.tamper_offsets(proof).items():
        bad = bytearray(proof)
        bad[off] ^= 0x04
        cases.append((name, bytes(bad)))
    for sec in CSA.element_sections(proof):
        cases.append((sec + ">=p", CSA.noncanonical(proof, sec)))
    cases.append(("truncated", proof[:-8]))
    cases.append(("truncated-in-header", proof[:100]))
    return o, w, cases


@pytest.mark.parametrize("ext", [0, 2])
def test_tampered_sections(backend, oracle, ext):
    """one bit flipped in every section, a word >= p in every element section, a truncated proof, other expected options; the batch
    answers as the single calls do, in any order"""
    o, w, cases = _tampered(ext)
    proof = cases[0][1]
    expect = [expected(p, w) for _, p in cases]
    got = schnorr_verify(backend, [(p, w) for _, p in cases])
    for (name, _), g, e in zip(cases, got, expect):
        assert g == e and (g != "OK") == (name != "honest"), (name, g, e)
    assert {"MALFORMED", "OOD", "TRACE_OPENING", "COMPOSITION_OPENING", "LAYER_OPENING", "REMAINDER_COMMITMENT"} <= set(got)
    assert [schnorr_verify(backend, [(p, w)])[0] for _, p in cases] == got
    order = np.random.default_rng(11).permutation(len(cases))
    assert [schnorr_verify(backend, [(cases[i][1], w) for i in order])[k] for k in np.argsort(order)] == got
    for field in range(7):
        e = list(o)
        e[field] = e[field] + 1 if field != 1 else 16
        assert schnorr_verify(backend, [(proof, w)], _opts(tuple(e))) == ["OPTIONS_MISMATCH"] == [CS.oracle_verdict(proof, w, e)], field


def test_header_values_no_prover_writes(backend, oracle):
    """a signature count that is not the trace's: MALFORMED whatever the statement says"""
    proof, w = CS.honest()
    cases = []
    for word in (0, 2, 3):
        bad = bytearray(proof)
        struct.pack_into("<I", bad, 20, word)
        cases.append((bytes(bad), w if word != 2 else CS.witness(2)))
    assert schnorr_verify(backend, cases) == ["MALFORMED"] * 3


# ---- 4. the cheating prover -------------------------------------------------------------------------------------------------------------
def test_cheating_prover_is_caught_by_the_isolating_check(backend, oracle):
    cases = CS.isolating_cases()
    assert schnorr_verify(backend, [CS.honest()]) == ["OK"]   # the control: the same prover without a deviation
    got = schnorr_verify(backend, [(proof, w) for proof, w, _, _ in cases.values()])
    for (name, (proof, w, verdict, _)), g in zip(cases.items(), got):
        assert g == verdict == CS.oracle_verdict(proof, w), (name, g)
    assert {"lying_statement:rx", "lying_statement:pkey", "lying_statement:msg", "shifted_deep"} <= set(cases) and "LAYER_FOLDING" in got


def test_mixed_batch(backend, oracle):
    """numbers of signatures, hashes, extensions and options mixed with rejected proofs: each verdict is the single call's"""
    cases = CS.isolating_cases()
    items = [CS.honest(), CS.honest(4, (8, 8, 0, 1, 1, 8, 256)), cases["lying_statement:pkey:2-signatures-cubic"][:2], CS.honest(2, (8, 8, 0, 0, 2, 4, 128)),
             cases["invalid_trace:limb"][:2], CS.honest(8, CS.OPTIONS), cases["shifted_deep"][:2], (CS.honest()[0], CS.witness(2))]
    batch = schnorr_verify(backend, items)
    assert batch == [schnorr_verify(backend, [it])[0] for it in items]
    assert batch == ["OK", "OK", "OOD", "OK", "OOD", "OK", "LAYER_FOLDING", "OOD"]
    assert batch[:7] == [CS.oracle_verdict(p, w) for p, w in items[:7]]


# ---- 5. proofs of another AIR -----------------------------------------------------------------------------------------------------------
def test_proofs_of_another_air(backend, oracle):
    merkle, _ = CSA.honest(CSA.MERKLE, CSA.OPTIONS[CSA.MERKLE])
    w = CS.witness()
    assert schnorr_verify(backend, [(merkle, w), (CSA.noncanonical(merkle, "trace_rows"), w), CS.honest()]) == ["UNSUPPORTED", "MALFORMED", "OK"]


# ---- 6. two chunks ----------------------------------------------------------------------------------------------------------------------
def test_batch_of_two_chunks(backend, oracle):
    """4096 entries of one 1-signature proof pass the staging budget of one chunk; one entry behind the boundary is tampered with"""
    proof, w = CS.honest()
    count, at = 4096, 3900
    assert count * (len(proof) + 304) > 64 << 20 and (at + 1) * (len(proof) + 2048) > 64 << 20 > 2048 * (len(proof) + 304)
    bad = bytearray(proof)
    bad[CSA.tamper_offsets(proof)["ood_cur"]] ^= 0x04
    proofs = [proof] * count
    proofs[at] = bytes(bad)
    got = backend.schnorr_verify(proofs, [w] * count)
    assert backend.verify_h2d_bytes() > count * (len(proof) + 304)
    assert names(got[[0, at - 1, at, at + 1, count - 1]]) == ["OK", "OK", "OOD", "OK", "OK"] and int((got != 0).sum()) == 1


def test_stage_times_and_copied_bytes(backend, oracle):
    proof, w = CS.honest()
    assert schnorr_verify(backend, [(proof, w)] * 3) == ["OK"] * 3
    three, ms = backend.verify_h2d_bytes(), backend.verify_stage_ms()
    assert 3 * (len(proof) + 304) < three < 3 * len(proof) + 65536 and all(v >= 0 for v in ms.values()) and ms["ood"] > 0
    assert schnorr_verify(backend, [(proof, w)]) == ["OK"]
    assert len(proof) + 304 < backend.verify_h2d_bytes() < three


# ---- 7. misuse --------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_a_status_not_a_verdict(backend, oracle):
    from certificate_stark_amd._lib import CstarkError, SchnorrStatementStruct, u64p, u8p
    proof, w = CS.honest()
    lib, ctx = backend.lib, backend.ctx
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    ptrs = (C.POINTER(C.c_uint8) * 1)(C.cast(buf, C.POINTER(C.c_uint8)))
    lens = (C.c_size_t * 1)(len(proof))
    msg, rx, s = np.ascontiguousarray(w.messages), np.ascontiguousarray(w.sig_rx), np.ascontiguousarray(w.sig_s)

    def stm(n_sig=1, messages=True, sig_rx=True, sig_s=True):
        st = (SchnorrStatementStruct * 1)()
        st[0].n_sig = n_sig
        st[0].messages = msg.ctypes.data_as(u64p) if messages else None
        st[0].sig_rx = rx.ctypes.data_as(u64p) if sig_rx else None
        st[0].sig_s = s.ctypes.data_as(u8p) if sig_s else None
        return st
    verdict = (C.c_int32 * 1)(-7)
    assert lib.cstark_schnorr_verify(ctx, C.c_uint32(1), ptrs, lens, stm(), None, verdict) == 0 and verdict[0] == 0
    for args in ((None, lens, stm(), None, verdict), (ptrs, None, stm(), None, verdict), (ptrs, lens, None, None, verdict), (ptrs, lens, stm(), None, None),
                 (ptrs, lens, stm(messages=False), None, verdict), (ptrs, lens, stm(sig_rx=False), None, verdict), (ptrs, lens, stm(sig_s=False), None, verdict),
                 (ptrs, lens, stm(n_sig=0), None, verdict)):
        assert lib.cstark_schnorr_verify(ctx, C.c_uint32(1), *args) < 0
    assert lib.cstark_schnorr_verify(None, C.c_uint32(1), ptrs, lens, stm(), None, verdict) < 0
    assert lib.cstark_schnorr_verify(ctx, C.c_uint32(0), None, None, None, None, None) == 0
    assert list(backend.schnorr_verify([], [])) == []
    for field, t, k in (("messages", 0, 0), ("messages", 0, 27), ("sig_rx", 0, 5)):
        bad = CS.changed(w, field, t, k)
        getattr(bad, field)[t, k] = P
        with pytest.raises(CstarkError):
            backend.schnorr_verify([proof], [bad])
    with pytest.raises(ValueError):
        backend.schnorr_verify([proof], [])
    assert schnorr_verify(backend, [(b"", w), (b"CSTK", w), (proof[:51], w)]) == ["MALFORMED"] * 3


def test_context_that_has_never_proved(oracle):
    from certificate_stark_amd.backend import Backend
    fresh = Backend()
    try:
        assert schnorr_verify(fresh, [CS.honest(), CS.honest(2, (8, 8, 0, 1, 1, 8, 256))]) == ["OK"] * 2
    finally:
        fresh.close()
