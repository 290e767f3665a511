"""cstark_tx_verify on the GPU: the reference's acceptance tests (src/tests.rs:11-38) with the product verifier, an option matrix,
tampering of every section with the verdict the restated verifier (oracle/verifier.py) implies, mixed batches, isolation from the
prover, and the headline proof."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 62) + (1 << 56) + (1 << 55) + 1
V_OK, V_MALFORMED, V_UNSUPPORTED, V_OPTIONS, V_OOD = 0, 1, 2, 3, 4


def _opts(t):
    from certificate_stark_amd.prover import ProofOptions
    return ProofOptions(*t)


def example(n_tx, depth, options, seed=0x5EED, backend=None):
    from oracle import oracle as O
    from certificate_stark_amd.prover import TransactionExample, TransactionMetadata
    w = O.TxWitness.generate(n_tx, depth, seed=seed)
    meta = TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS])
    return TransactionExample(_opts(options), meta, backend)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def oracle_verdict(proof, r0, r1, options=None):
    """the restated verifier's reason, mapped to the verdict names of include/cstark.h"""
    from oracle import verifier as Vf
    try:
        Vf.verify(proof, r0, r1, options=options)
        return "OK"
    except Vf.VerifierError as e:
        msg = str(e)
    table = [("not a TransactionAir proof", "UNSUPPORTED"), ("proof options differ", "OPTIONS_MISMATCH"), ("out-of-domain", "OOD"),
             ("does not match its commitment", None), ("proof of work", "POW"), ("trace opening", "TRACE_OPENING"),
             ("composition opening", "COMPOSITION_OPENING"), ("wrong number", "LAYER_COUNT"), ("opening does not match", "LAYER_OPENING"),
             ("evaluation differs", "LAYER_FOLDING"), ("remainder differs", "REMAINDER_FOLDING"), ("low-degree", "REMAINDER_DEGREE")]
    if msg.startswith("remainder does not match its commitment"):
        return "REMAINDER_COMMITMENT"
    for key, name in table:
        if key in msg and name:
            return name
    return "MALFORMED"


def names(verdicts):
    from certificate_stark_amd import VERDICTS
    return [VERDICTS[int(v)] for v in verdicts]


def words_canonical(proof):
    """every 8-byte word of every element section below p (proof layout of include/cstark.h)"""
    from certificate_stark_amd import inspect_proof
    info = inspect_proof(proof)
    if info.verdict != 0:
        return True  # the layout decides first
    nq, blowup, _, _, ext, fold, _ = info.options
    m, W, ce = ext + 1, info.trace_width, {94: 8, 65: 4, 56: 8, 2: 2, 14: 4}[info.trace_width]
    log_N, log_f = info.log_n + blowup.bit_length() - 1, fold.bit_length() - 1
    nl = struct.unpack_from("<I", proof, 116)[0]
    secs = []
    o = 152 + 32 * nl
    secs.append((o, (2 * W + ce) * m)); o += 8 * (2 * W + ce) * m + 8
    secs.append((o, nq * W)); o += 8 * nq * W + 32 * nq * log_N
    secs.append((o, nq * ce * m)); o += 8 * nq * ce * m + 32 * nq * log_N
    lg = log_N
    for _ in range(nl):
        npos = struct.unpack_from("<I", proof, o)[0]; o += 4
        secs.append((o, npos * fold * m)); o += 8 * npos * fold * m + 32 * npos * (lg - log_f)
        lg -= log_f
    rl = struct.unpack_from("<I", proof, o)[0]; o += 4
    secs.append((o, rl * m))
    return all(np.all(np.frombuffer(proof, np.uint64, n, off) < P) for off, n in secs if n)


# ---- the reference's acceptance tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [0, 1, 2])
def test_transaction_proof_verification(backend, ext):
    tx = example(2, 3, (42, 8, 0, 0, ext, 4, 256), backend=backend)
    proof = tx.prove()
    tx.verify(proof)  # raises VerifierError on rejection


def test_transaction_proof_verification_fail(backend):
    """verify_with_wrong_inputs (src/lib.rs:152-161) in both forms of tests/test_gpu_prove.py"""
    from certificate_stark_amd import VerifierError
    tx = example(2, 3, (42, 8, 0, 0, 0, 4, 256), backend=backend)
    proof = tx.prove()
    r0, r1 = tx.pub_inputs()
    v = backend.tx_verify([proof, proof], [r0, r1], [np.full(7, r1[0], np.uint64), r1])
    assert names(v) == ["OOD", "OOD"]
    tx.tx_metadata.final_root = np.full(7, r1[0], np.uint64)
    with pytest.raises(VerifierError) as e:
        tx.verify(proof)
    assert e.value.reason == "OOD" and e.value.verdict == V_OOD


def test_golden_proof_is_accepted(backend):
    z = np.load(os.path.join(ROOT, "tests", "golden", "proof_2tx_d3.npz"))
    proof = z["proof"].tobytes()
    assert list(backend.tx_verify([proof], z["initial_root"], z["final_root"], _opts((42, 8, 0, 0, 0, 4, 256)))) == [V_OK]


# ---- option matrix --------------------------------------------------------------------------------------------------------------
MATRIX = [
    (1, 3, (42, 8, 0, 0, 0, 4, 256)),
    (2, 3, (1, 8, 0, 1, 0, 4, 128)),
    (2, 3, (128, 16, 0, 0, 1, 8, 1024)),
    (4, 3, (24, 8, 3, 1, 2, 16, 512)),
    (2, 15, (32, 8, 0, 0, 2, 4, 256)),
    (16, 3, (16, 8, 2, 0, 0, 8, 256)),
    (2, 3, (20, 16, 12, 0, 0, 16, 128)),
    (8, 15, (12, 8, 0, 1, 1, 4, 1024)),
]


@pytest.fixture(scope="module")
def matrix_proofs(backend):
    out = []
    for n_tx, depth, o in MATRIX:
        tx = example(n_tx, depth, o, backend=backend)
        out.append((tx.prove(), *tx.pub_inputs(), o))
    return out


def test_option_matrix_accepted(backend, matrix_proofs):
    from oracle import verifier as Vf
    for proof, r0, r1, o in matrix_proofs:
        assert Vf.verify(proof, r0, r1, options=list(o))
        assert list(backend.tx_verify([proof], r0, r1)) == [V_OK], o
        assert list(backend.tx_verify([proof], r0, r1, _opts(o))) == [V_OK], o


def test_option_mismatch(backend, matrix_proofs):
    proof, r0, r1, o = matrix_proofs[3]
    for field in range(7):
        e = list(o)
        e[field] = e[field] + 1 if field != 1 else 16
        assert names(backend.tx_verify([proof], r0, r1, _opts(tuple(e)))) == ["OPTIONS_MISMATCH"], field


# ---- tampering --------------------------------------------------------------------------------------------------------------------
def _tamper_offsets(proof):
    from certificate_stark_amd import inspect_proof
    info = inspect_proof(proof)
    nq, blowup, _, _, ext, fold, _ = info.options
    m, W, ce = ext + 1, 94, 8
    log_N, log_f = info.log_n + blowup.bit_length() - 1, fold.bit_length() - 1
    nl = struct.unpack_from("<I", proof, 116)[0]
    offs = {"trace_root": 53, "cons_root": 90, "layer_root_0": 121, "layer_root_last": 120 + 32 * (nl - 1) + 17,
            "rem_commit": 120 + 32 * nl + 5}
    o = 152 + 32 * nl
    offs["ood_cur"] = o + 8 * 59 + 2
    offs["ood_next"] = o + 8 * W * m + 8 * 3
    offs["ood_comp"] = o + 8 * 2 * W * m + 8 * 5 + 1
    o += 8 * (2 * W + ce) * m
    offs["nonce"] = o + 1
    o += 8
    offs["trace_row"] = o + 8 * (W * 3 + 17) + 2
    o += 8 * nq * W
    offs["trace_path"] = o + 32 * (log_N * 2 + 5) + 7
    o += 32 * nq * log_N
    offs["cons_row"] = o + 8 * (ce * m * 1 + 3)
    o += 8 * nq * ce * m
    offs["cons_path"] = o + 32 * (log_N * 1 + 2) + 9
    o += 32 * nq * log_N
    lg = log_N
    for l in range(nl):
        npos = struct.unpack_from("<I", proof, o)[0]
        o += 4
        if l in (0, nl - 1):
            offs["layer%d_row" % l] = o + 8 * (fold * m * (npos - 1) + 1) + 3
        o += 8 * npos * fold * m
        if l in (0, nl - 1):
            offs["layer%d_path" % l] = o + 32 * (lg - log_f) * (npos // 2) + 4
        o += 32 * npos * (lg - log_f)
        lg -= log_f
    rl = struct.unpack_from("<I", proof, o)[0]
    offs["remainder"] = o + 4 + 8 * (rl // 3) + 2
    return offs


@pytest.mark.parametrize("cfg", [(2, 3, (24, 8, 0, 0, 0, 4, 256)), (2, 3, (24, 8, 4, 1, 2, 8, 256))])
def test_tampered_sections(backend, cfg):
    n_tx, depth, o = cfg
    tx = example(n_tx, depth, o, backend=backend)
    proof = tx.prove()
    r0, r1 = tx.pub_inputs()
    bads, expect = [], []
    for name, off in _tamper_offsets(proof).items():
        for bit in (0x01, 0x80):
            bad = bytearray(proof)
            bad[off] ^= bit
            bad = bytes(bad)
            bads.append((name, bad))
            expect.append(oracle_verdict(bad, r0, r1) if words_canonical(bad) else "MALFORMED")
    got = names(backend.tx_verify([b for _, b in bads], r0, r1))
    for (name, _), g, e in zip(bads, got, expect):
        assert g != "OK", name
        assert g == e, (name, g, e)


def test_tampered_header_words(backend):
    o = (24, 8, 0, 0, 0, 4, 256)
    tx = example(2, 3, o, backend=backend)
    proof = tx.prove()
    r0, r1 = tx.pub_inputs()
    allowed = {0: {"MALFORMED"}, 4: {"MALFORMED"}, 8: {"MALFORMED", "UNSUPPORTED"}, 12: {"MALFORMED"}, 16: {"MALFORMED"}}
    for k in range(7):
        allowed[24 + 4 * k] = {"MALFORMED", "OPTIONS_MISMATCH"}
    cases = []
    for off, ok in allowed.items():
        for bit in (0x01, 0x02, 0x10):
            bad = bytearray(proof)
            bad[off] ^= bit
            cases.append((off, bytes(bad), ok))
    for depth, ok in ((7, {"OOD"}), (15, {"OOD"}), (4, {"MALFORMED"}), (2, {"MALFORMED"})):  # the Merkle-depth word
        bad = bytearray(proof)
        struct.pack_into("<I", bad, 20, depth)
        cases.append((20, bytes(bad), ok))
    got = names(backend.tx_verify([b for _, b, _ in cases], r0, r1, _opts(o)))
    for (off, _, ok), g in zip(cases, got):
        assert g in ok, (off, g)


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_equals_single_calls(backend, matrix_proofs, oracle):
    from oracle import prover as OP
    items = []
    for i, (proof, r0, r1, o) in enumerate(matrix_proofs):
        items.append((proof, r0, r1))
        bad = bytearray(proof)
        bad[len(proof) - 8 * (i + 1) - 3] ^= 0x04   # the remainder
        items.append((bytes(bad), r0, r1))
    items.append(items[0])                              # duplicates
    items.append(items[4])
    w = oracle.TxWitness.generate(2, 3, seed=0x5EED)
    merkle = OP.prove_air(oracle.AIR_MERKLE, w, (8, 8, 0, 0, 0, 4, 128))
    items.insert(3, (merkle, w.initial_roots[0], w.final_root))
    assert len(items) >= 12
    proofs = [p for p, _, _ in items]
    r0s = np.stack([np.asarray(r, np.uint64) for _, r, _ in items])
    r1s = np.stack([np.asarray(r, np.uint64) for _, _, r in items])
    batch = names(backend.tx_verify(proofs, r0s, r1s))
    single = [names(backend.tx_verify([p], a, b))[0] for p, a, b in items]
    assert batch == single
    assert batch[3] == "UNSUPPORTED"
    expect = [oracle_verdict(p, a, b) if words_canonical(p) else "MALFORMED" for p, a, b in items]
    assert batch == expect
    assert batch.count("OK") == len(matrix_proofs) + 2
    assert list(backend.tx_verify([], r0s[:0], r1s[:0])) == []


# ---- isolation --------------------------------------------------------------------------------------------------------------------
def test_verify_does_not_disturb_the_prover(backend, oracle):
    from certificate_stark_amd.prover import MerkleExample, TransactionMetadata
    from oracle import verifier as Vf
    tx = example(2, 3, (42, 8, 0, 0, 0, 4, 256), backend=backend)
    p1 = tx.prove()
    other = example(4, 3, (16, 8, 0, 1, 2, 8, 128), seed=3, backend=backend)
    p_other = other.prove()
    assert names(backend.tx_verify([p1, p_other], np.stack([tx.pub_inputs()[0], other.pub_inputs()[0]]),
                                   np.stack([tx.pub_inputs()[1], other.pub_inputs()[1]]))) == ["OK", "OK"]
    assert tx.prove() == p1
    # a resident witness (MerkleExample keeps its upload) still proves correctly after a verification
    w = oracle.TxWitness.generate(2, 3, seed=5)
    meta = TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS])
    mex = MerkleExample(_opts((8, 8, 0, 0, 0, 4, 128)), meta, backend)
    m1 = mex.prove()
    backend.tx_verify([p1], *tx.pub_inputs())
    assert mex.prove() == m1
    assert Vf.verify_merkle(m1, w.initial_roots[0], w.final_root)


# ---- headline size ----------------------------------------------------------------------------------------------------------------
def test_headline_proof(backend):
    from certificate_stark_amd.prover import TransactionExample, TransactionMetadata
    meta = TransactionMetadata.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))
    o = (96, 8, 0, 0, 0, 4, 256)
    tx = TransactionExample(_opts(o), meta, backend)
    proof = tx.prove()
    r0, r1 = tx.pub_inputs()
    bad = bytearray(proof)
    bad[len(proof) - 100] ^= 0x20
    assert names(backend.tx_verify([proof, bytes(bad)], r0, r1, _opts(o)))[0] == "OK"
    assert names(backend.tx_verify([bytes(bad)], r0, r1))[0] != "OK"
