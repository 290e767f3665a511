"""GPU: conversion of proofs between the plain and the compact form (cstark_tx_convert, cstark_air_convert, cstark_schnorr_convert;
k_vfy_multi_select and k_vfy_multi_expand in csrc/verify.hip).

A convert call is its verify call that also writes every accepted proof in the other form.  The plain -> compact result must be the
Python reference's selection (tests/compact_cases.py: compact) from the CPU prover's plain proof, the compact -> plain result that
plain proof again, byte for byte; the verdicts must be the verify call's; a refused proof is not converted and its buffer not written.
Shapes as in tests/test_gpu_compact_proofs.py: two transfers at Merkle depth 3 and 64-row range proofs, at option sets that cover
Blake3 and Sha3, the three extension degrees, folding 4, 8 and 16, proofs without a FRI layer, 128 queries into a 256-leaf tree and a
64-leaf layer tree with 61 leaves opened under 3 nodes."""
import ctypes as C
import struct

import numpy as np
import pytest

import compact_cases as CC

pytestmark = pytest.mark.gpu

P = (1 << 62) + (1 << 56) + (1 << 55) + 1
INPUTS = [("tx", o) for o in CC.TX_OPTS] + [("range", o) for o in CC.RANGE_OPTS]
FILL = 0xA5


def metadata(w):
    from certificate_stark_amd.prover import TransactionMetadata
    return TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS])


def options(opts):
    from certificate_stark_amd.prover import ProofOptions
    return ProofOptions(*opts)


def names(verdicts):
    from certificate_stark_amd import VERDICTS
    return [VERDICTS[int(v)] for v in verdicts]


@pytest.fixture(scope="module")
def backend(oracle):
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def case(kind, opts):
    return CC.tx_case(2, 3, opts) if kind == "tx" else CC.range_case(opts)


def convert(backend, kind, proofs, form, options=None):
    if kind == "tx":
        w = CC.witness(2, 3)
        return backend.tx_convert(proofs, w.initial_roots[0], w.final_root, form, options=options)
    return backend.air_convert(proofs, backend.AIR_RANGE, form=form, numbers=CC.range_number(), options=options)


def verify(backend, kind, proofs, options=None):
    if kind == "tx":
        w = CC.witness(2, 3)
        return backend.tx_verify(proofs, w.initial_roots[0], w.final_root, options=options)
    return backend.air_verify(proofs, backend.AIR_RANGE, numbers=CC.range_number(), options=options)


def flip(proof, at, bit=0x10):
    b = bytearray(proof)
    b[at] ^= bit
    return bytes(b)


# ---- 1: both directions against the Python reference (the test that fails without the feature) -------------------------------------
@pytest.mark.parametrize("kind,opts", INPUTS)
def test_both_directions_equal_the_reference(oracle, backend, kind, opts):
    plain, positions = case(kind, opts)
    compact = CC.compact(plain, positions)
    got, verdicts = convert(backend, kind, [plain], "compact")
    assert names(verdicts) == ["OK"]
    assert len(got[0]) == len(compact)
    assert got[0] == compact
    back, verdicts = convert(backend, kind, [compact], "plain")
    assert names(verdicts) == ["OK"]
    assert len(back[0]) == len(plain)
    assert back[0] == plain
    assert names(verify(backend, kind, [got[0], back[0]])) == ["OK", "OK"]
    # both in one call, and a proof already in the target form comes back as it is
    for form, want in (("compact", compact), ("plain", plain)):
        both, verdicts = convert(backend, kind, [plain, compact], form)
        assert names(verdicts) == ["OK", "OK"] and both == [want, want]


# ---- 2: one call, every mix ---------------------------------------------------------------------------------------------------------
def test_one_call_converts_every_air_hash_and_extension(oracle, backend):
    """the statements of test_compact_sub_air_proofs_are_accepted (tests/test_gpu_compact_proofs.py) and a TransactionAir proof: Blake3
    and Sha3, base field, quadratic and cubic; every output is the example's own prove() / prove(compact=True)"""
    from certificate_stark_amd.prover import MerkleExample, RangeProofExample, RescueExample, SchnorrExample, TransactionExample
    po = options((42, 8, 0, 0, 0, 4, 256))
    w = CC.witness(2, 3)
    tex = TransactionExample(po, metadata(w), backend)
    mex = MerkleExample(po, metadata(w), backend)
    rex = RescueExample(8, options((20, 4, 0, 1, 1, 4, 128)), backend)
    number = CC.range_number()
    gex = RangeProofExample(options(CC.RANGE_OPTS[3]), number, backend)
    proofs, airs, pubs, plains, compacts = [], [], [], [], []
    for ex, air, pub in ((tex, backend.AIR_TRANSACTION, np.concatenate(tex.pub_inputs())), (mex, backend.AIR_MERKLE, np.concatenate(mex.pub_inputs())),
                         (rex, backend.AIR_RESCUE_CHAIN, np.concatenate(rex.pub_inputs())), (gex, backend.AIR_RANGE, np.array([number] + [0] * 13, np.uint64))):
        plain, compact = ex.prove(), ex.prove(compact=True)
        assert plain[:4] == b"CSTK" and compact[:4] == b"CSTC"
        proofs += [compact, plain]; airs += [air, air]; pubs += [pub, pub]
        plains += [plain, plain]; compacts += [compact, compact]
        assert ex.convert(plain) == compact and ex.convert(compact, compact=False) == plain         # the examples' own surface
    pubs = np.array(pubs, np.uint64)
    got, verdicts = backend.air_convert(proofs, airs, pubs, form="compact")
    assert names(verdicts) == ["OK"] * 8 and got == compacts
    got, verdicts = backend.air_convert(proofs, airs, pubs, form="plain")
    assert names(verdicts) == ["OK"] * 8 and got == plains
    sex = SchnorrExample.build_random(po, 1, seed=91, backend=backend)
    plain, compact = sex.prove(), sex.prove(compact=True)
    got, verdicts = backend.schnorr_convert([compact, plain], [sex, sex], "compact")
    assert names(verdicts) == ["OK", "OK"] and got == [compact, compact]
    got, verdicts = backend.schnorr_convert([compact, plain], [sex, sex], "plain")
    assert names(verdicts) == ["OK", "OK"] and got == [plain, plain]
    assert sex.convert(plain) == compact and sex.convert(compact, compact=False) == plain
    # a SchnorrAir proof through air_convert: no statement to verify it against
    got, verdicts = backend.air_convert([plain, compact], backend.AIR_SCHNORR, np.zeros(14, np.uint64), form="compact")
    assert names(verdicts) == ["UNSUPPORTED", "UNSUPPORTED"] and got == [None, None]


# ---- 3: refused proofs --------------------------------------------------------------------------------------------------------------
def damaged(opts):
    """(what, proof, final root or None for the right one, verdict) -- damaged proofs between valid ones"""
    w = CC.witness(2, 3)
    plain, positions = CC.tx_case(2, 3, opts)
    good = CC.compact(plain, positions)
    trees, ptrees = CC.walk(good)[1], CC.walk(plain)[1]
    assert len(trees) >= 3 and all(t.n_nodes >= 2 for t in trees)
    fewer = bytearray(good[:trees[2].end - 32] + good[trees[2].end:])
    struct.pack_into("<I", fewer, trees[2].paths - 4, trees[2].n_nodes - 1)
    row_word = trees[0].rows + 8 * (94 * 5 + 3)
    not_canonical = bytearray(good)
    struct.pack_into("<Q", not_canonical, row_word, P)
    wrong_root = np.array(w.final_root, np.uint64).copy()
    wrong_root[2] = (int(wrong_root[2]) + 1) % P
    return [("valid compact", good, None, "OK"),
            ("a flipped node of the trace tree", flip(good, trees[0].paths + 32 * (trees[0].n_nodes // 2) + 7), None, "TRACE_OPENING"),
            ("valid plain", plain, None, "OK"),
            ("one node fewer in layer 0", bytes(fewer), None, "LAYER_OPENING"),
            ("a flipped path byte of the composition tree", flip(plain, ptrees[1].paths + 32 * 7 + 3), None, "COMPOSITION_OPENING"),
            ("a trace row word set to p", bytes(not_canonical), None, "MALFORMED"),
            ("valid compact under a wrong final root", good, wrong_root, "OOD"),
            ("valid plain under a wrong final root", plain, wrong_root, "OOD"),
            ("valid compact again", good, None, "OK")]


def roots_of(cases):
    w = CC.witness(2, 3)
    initial = np.array([w.initial_roots[0]] * len(cases), np.uint64)
    final = np.array([w.final_root if r is None else r for _, _, r, _ in cases], np.uint64)
    return initial, final


def raw_tx_convert(backend, proofs, initial, final, form, capacities=None, opts=None):
    """cstark_tx_convert at the ctypes level: every buffer holds its bound (or capacities[i]) and is filled with 0xA5 before the call
    -> (status, buffers as bytes, out_lens, verdicts)"""
    from certificate_stark_amd.verify import convert_bound
    count = len(proofs)
    keep = [bytes(p) for p in proofs]
    ptrs, lens = (C.POINTER(C.c_uint8) * count)(), (C.c_size_t * count)()
    out, caps, out_lens = (C.POINTER(C.c_uint8) * count)(), (C.c_size_t * count)(), (C.c_size_t * count)(*([12345] * count))
    bufs = []
    for i, p in enumerate(keep):
        ptrs[i], lens[i] = C.cast(C.c_char_p(p), C.POINTER(C.c_uint8)), len(p)
        cap = convert_bound(p, form) if capacities is None else capacities[i]
        bufs.append((C.c_uint8 * cap).from_buffer_copy(bytes([FILL]) * cap))
        out[i], caps[i] = C.cast(bufs[i], C.POINTER(C.c_uint8)), cap
    ir, fr = np.ascontiguousarray(initial, np.uint64), np.ascontiguousarray(final, np.uint64)
    verdicts = np.full(count, -9, np.int32)
    o = None if opts is None else C.byref(backend._options_struct(options(opts)))
    u64p = C.POINTER(C.c_uint64)
    rc = backend.lib.cstark_tx_convert(backend.ctx, count, ptrs, lens, ir.ctypes.data_as(u64p), fr.ctypes.data_as(u64p), o,
                                       backend.PROOF_FORMS.index(form), out, caps, out_lens, verdicts.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, [bytes(b) for b in bufs], list(out_lens), verdicts


@pytest.mark.parametrize("opts", [CC.TX_OPTS[0], CC.TX_OPTS[1]])
def test_refused_proofs_are_not_converted(oracle, backend, opts):
    """Blake3, then Sha3: the damaged proofs beside valid ones in ONE call, then each alone"""
    cases = damaged(opts)
    proofs = [p for _, p, _, _ in cases]
    initial, final = roots_of(cases)
    want = names(backend.tx_verify(proofs, initial, final))
    assert [(what, v) for (what, _, _, _), v in zip(cases, want)] == [(what, v) for what, _, _, v in cases]
    plain, positions = CC.tx_case(2, 3, opts)
    reference = {"plain": plain, "compact": CC.compact(plain, positions)}
    for form in ("compact", "plain"):
        got, verdicts = backend.tx_convert(proofs, initial, final, form)
        assert names(verdicts) == want
        assert got == [reference[form] if v == "OK" else None for v in want]
        rc, bufs, lens, verdicts = raw_tx_convert(backend, proofs, initial, final, form)
        assert rc == 0 and names(verdicts) == want
        for buf, n, v in zip(bufs, lens, want):
            if v == "OK":
                assert buf[:n] == reference[form] and set(buf[n:]) <= {FILL}
            else:
                assert n == 0 and set(buf) == {FILL}
    # alone: the verdict does not depend on the neighbours
    for i, (what, proof, _, verdict) in enumerate(cases):
        got, verdicts = backend.tx_convert([proof], initial[i], final[i], "plain" if proof[:4] == b"CSTC" else "compact")
        assert names(verdicts) == [verdict], what
        assert (got[0] is None) == (verdict != "OK"), what


# ---- 4: verdict parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expected", [None, CC.TX_OPTS[0], CC.TX_OPTS[2]])
def test_verdicts_are_the_verify_calls(oracle, backend, expected):
    """the case list of the refused proofs and the inputs of the first test, in both forms, with and without options="""
    po = None if expected is None else options(expected)
    cases = damaged(CC.TX_OPTS[0]) + damaged(CC.TX_OPTS[1])
    proofs = [p for _, p, _, _ in cases]
    initial, final = roots_of(cases)
    for opts in CC.TX_OPTS:
        plain, positions = CC.tx_case(2, 3, opts)
        proofs += [plain, CC.compact(plain, positions)]
    w = CC.witness(2, 3)
    extra = len(proofs) - len(cases)
    initial = np.concatenate([initial, np.array([w.initial_roots[0]] * extra, np.uint64)])
    final = np.concatenate([final, np.array([w.final_root] * extra, np.uint64)])
    want = names(backend.tx_verify(proofs, initial, final, options=po))
    assert ("OPTIONS_MISMATCH" in want) == (expected is not None)
    assert "OK" in want
    for form in ("compact", "plain"):
        got, verdicts = backend.tx_convert(proofs, initial, final, form, options=po)
        assert names(verdicts) == want
        assert [g is None for g in got] == [v != "OK" for v in want]
    ranges = []
    for opts in CC.RANGE_OPTS:
        plain, positions = CC.range_case(opts)
        ranges += [plain, CC.compact(plain, positions)]
    ro = None if expected is None else options(CC.RANGE_OPTS[3])
    want = names(verify(backend, "range", ranges, options=ro))
    assert want.count("OK") == (10 if expected is None else 2)
    for form in ("compact", "plain"):
        got, verdicts = convert(backend, "range", ranges, form, options=ro)
        assert names(verdicts) == want
        assert [g is None for g in got] == [v != "OK" for v in want]


# ---- 5: capacities ------------------------------------------------------------------------------------------------------------------
def test_a_short_capacity_is_refused_before_any_launch(oracle, backend):
    from certificate_stark_amd.verify import convert_bound
    opts = CC.TX_OPTS[0]
    w = CC.witness(2, 3)
    plain, positions = CC.tx_case(2, 3, opts)
    compact = CC.compact(plain, positions)
    trees = len(CC.walk(plain)[1])
    assert convert_bound(plain, "compact") == len(plain) + 4 * trees >= len(compact)
    assert convert_bound(compact, "plain") == len(plain)
    proofs = [plain, compact, plain]
    initial, final = np.array([w.initial_roots[0]] * 3, np.uint64), np.array([w.final_root] * 3, np.uint64)
    for form in ("compact", "plain"):
        caps = [convert_bound(p, form) for p in proofs]
        caps[1] -= 1
        rc, bufs, lens, verdicts = raw_tx_convert(backend, proofs, initial, final, form, capacities=caps)
        assert rc == -1                                                                            # CSTARK_ERR_INVALID_ARG
        assert b"proof 1" in backend.lib.cstark_last_error()
        assert all(set(b) == {FILL} for b in bufs) and list(verdicts) == [-9] * 3 and lens == [12345] * 3
        # the context is as it was: the same call with the bound works
        rc, bufs, lens, verdicts = raw_tx_convert(backend, proofs, initial, final, form)
        want = compact if form == "compact" else plain
        assert rc == 0 and names(verdicts) == ["OK"] * 3 and lens == [len(want)] * 3
        assert all(b[:len(want)] == want for b in bufs)
    # misuse: another form, null outputs
    v = (C.c_int32 * 1)()
    assert backend.lib.cstark_tx_convert(backend.ctx, 1, None, None, None, None, None, 2, None, None, None, v) == -1
    rc, bufs, lens, verdicts = raw_tx_convert(backend, [plain], initial[:1], final[:1], "compact")
    assert rc == 0
    with pytest.raises(ValueError):
        backend.tx_convert([plain], initial[0], final[0], "short")


# ---- 6: the context proves and verifies on ---------------------------------------------------------------------------------------------
def test_the_context_proves_and_verifies_on(oracle):
    from certificate_stark_amd.backend import Backend
    opts = CC.TX_OPTS[0]
    w = CC.witness(2, 3)
    plain, positions = CC.tx_case(2, 3, opts)
    compact = CC.compact(plain, positions)
    roots = (w.initial_roots[0], w.final_root)
    b = Backend()
    try:
        b.upload_witness(metadata(w))
        assert names(b.tx_verify([plain], *roots)) == ["OK"]
        h2d = b.verify_h2d_bytes()
        assert b.prove(options(opts)) == plain
        assert b.tx_convert([plain], *roots, "compact")[0] == [compact]
        assert b.proof_form == "plain" and b.prove_channel() == "device"
        b.proof_form = "compact"
        assert b.prove(options(opts)) == compact
        assert b.tx_convert([compact], *roots, "plain")[0] == [plain]
        assert b.proof_form == "compact" and b.prove_channel() == "device"
        assert b.prove(options(opts)) == compact                       # the witness is still resident, the form still set
        b.proof_form = "plain"
        assert b.prove(options(opts)) == plain
        assert b.prove_channel() == "device"
        assert names(b.tx_verify([plain], *roots)) == ["OK"]
        assert b.verify_h2d_bytes() == h2d
        stages = b.verify_stage_ms()
        assert set(stages) == {"host", "h2d", "transcript", "ood", "openings", "fri", "remainder_reduce_d2h"}
    finally:
        b.close()
