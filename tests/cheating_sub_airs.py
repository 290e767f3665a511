"""Sub-AIR proofs by a prover that cheats -- builders shared by test_oracle_sub_air_cheats.py (CPU) and test_gpu_air_verify.py (GPU),
in the manner of cheating_prover.py: the CPU prover (oracle/prover.py) with ONE step altered and everything after it honest.

  invalid_trace     one trace cell + 1, honestly committed                         -> only the out-of-domain equation (OOD)
  lying_statement   public() states a final root / result / number that is one off -> only the boundary terms of that equation (OOD)
  shifted_deep      DEEP evaluations + 1 before they are committed                 -> LAYER_FOLDING at layer 0, or -- a proof without a
                                                                                      FRI layer -- REMAINDER_FOLDING

and the byte-level view of a proof of any AIR (sections, tamper offsets, words >= p).  Not a conftest: nothing here changes how tests
are collected."""
import functools
import struct

import numpy as np

from cheating_prover import P, _Patched, _add, _one

MERKLE, SCHNORR, RANGE, RESCUE = 1, 2, 3, 4
SHAPE = {0: (94, 8), MERKLE: (65, 4), SCHNORR: (56, 8), RANGE: (2, 2), RESCUE: (14, 4)}   # AIR -> trace width, composition columns
NAMES = {0: "transaction", MERKLE: "merkle", RANGE: "range", RESCUE: "rescue"}

# cells (column, row) every one of which a constraint of its AIR binds (never row 0 or the last row: public() reads the statement there)
CELLS = {MERKLE: [(3, 5), (60, 100), (0, 1), (64, 17)], RANGE: [(0, 10), (1, 10), (1, 62)], RESCUE: [(3, 5), (10, 33), (0, 62)]}
# the smallest shapes: 1 transfer at depth 3 (2^9 rows), a 64-row range proof, a chain of 8 hashes (64 rows)
OPTIONS = {MERKLE: (8, 4, 0, 0, 0, 4, 128), RANGE: (8, 8, 0, 0, 0, 4, 128), RESCUE: (8, 4, 0, 0, 0, 4, 128)}
NUMBER = 0x1234_5678_9ABC_DEF0 >> 2   # canonical value of the range statement, below 2^63


def mont(v):
    from oracle import verifier as V
    return V.to_mont(v)


def rescue_seed():
    return np.array([mont(v) for v in range(42, 49)], np.uint64)   # benches/rescue.rs:25-31


def witness(air, n_tx=1, depth=3):
    """what oracle.prover's job of `air` is built from"""
    from oracle import oracle as O
    if air == MERKLE:
        return (O.TxWitness.generate(n_tx, depth, seed=0x5EED),)
    if air == RANGE:
        return (mont(NUMBER),)
    return (rescue_seed(), 8)


def job_class(air):
    from oracle import prover as OP
    return {MERKLE: OP.MerkleJob, RANGE: OP.RangeJob, RESCUE: OP.RescueJob}[air]


def prove(job, options):
    from oracle import prover as OP
    return OP._prove_job(job, tuple(options))


def statement(job):
    """the 14 public words cstark_air_verify takes for the proof a job made (memory form; RangeProofAir: the number, then zeros)"""
    pub = np.zeros(14, np.uint64)
    words = job.stated
    pub[:len(words)] = words
    return pub


def _recording(cls):
    """cls whose public() also keeps what it returned, as job.stated"""
    class Job(cls):
        def public(self, trace):
            words, extra = cls.public(self, trace)
            self.stated = [int(v) for v in words]
            return words, extra
    return Job


def honest(air, options, wit=None):
    job = _recording(job_class(air))(*(wit or witness(air)))
    return prove(job, options), statement(job)


def verify(air, proof, pub, options=None):
    """the restated verifier of `air` (raises its VerifierError)"""
    from oracle import verifier as V
    pub = np.asarray(pub, np.uint64)
    if air == MERKLE:
        return V.verify_merkle(proof, pub[:7], pub[7:], options=options)
    if air == RANGE:
        return V.verify_range(proof, int(pub[0]), options=options)
    if air == RESCUE:
        return V.verify_rescue(proof, pub[:7], pub[7:], options=options)
    return V.verify(proof, pub[:7], pub[7:], options=options)


# ---- the three deviations -------------------------------------------------------------------------------------------------------------
def invalid_trace(air, options, col, row):
    base = _recording(job_class(air))

    class Job(base):
        def build(self):
            trace = base.build(self)
            assert 0 < row < trace.shape[1] - 1, "rows 0 and n - 1 carry the statement"
            trace[col, row] = (int(trace[col, row]) + _one()) % P
            return trace
    job = Job(*witness(air))
    return prove(job, options), statement(job)


def lying_statement(air, options):
    """public() states a final root / result / number one above what the trace holds: the channel is seeded with the lie and the proof is
    verified against it, the boundary quotients were built from the trace's own values"""
    base = job_class(air)
    word = 0 if air == RANGE else 7

    class Job(base):
        def public(self, trace):
            words, extra = base.public(self, trace)
            words = [int(v) for v in words]
            words[word] = (words[word] + _one()) % P
            self.stated = words
            return words, extra
    job = Job(*witness(air))
    return prove(job, options), statement(job)


def shifted_deep(air, options, component=0):
    m = options[4] + 1

    def wrap(call, out):
        if m == 1:
            return _add(out, _one())
        out = np.array(out, np.uint64, copy=True)
        out[component] = _add(out[component], _one())
        return out
    job = _recording(job_class(air))(*witness(air))
    with _Patched("deep_composition_ext" if m > 1 else "deep_composition", wrap) as pt:
        proof = prove(job, options)
    assert pt.calls == 1
    return proof, statement(job)


@functools.lru_cache(maxsize=None)
def isolating_cases():
    """name -> (AIR, proof, public words, the one verdict that rejects it, a part of the restated verifier's message)"""
    cases = {}
    for air in (MERKLE, RANGE, RESCUE):
        for col, row in CELLS[air]:
            cases["invalid_trace:%s:%d,%d" % (NAMES[air], col, row)] = (air, *invalid_trace(air, OPTIONS[air], col, row), "OOD", "out-of-domain")
        cases["lying_statement:" + NAMES[air]] = (air, *lying_statement(air, OPTIONS[air]), "OOD", "out-of-domain")
    cases["shifted_deep:one-layer"] = (RANGE, *shifted_deep(RANGE, (8, 8, 0, 0, 2, 4, 128)), "LAYER_FOLDING", "layer 0: evaluation differs")
    cases["shifted_deep:no-layer"] = (RANGE, *shifted_deep(RANGE, (8, 4, 0, 0, 0, 4, 256)), "REMAINDER_FOLDING", "remainder differs")
    return cases


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------
def layout(proof):
    """section offsets of a proof of any AIR (layout of include/cstark.h), from its header and count words"""
    air, width, log_n = struct.unpack_from("<3I", proof, 8)
    nq, blowup, _, _, ext, fold, _ = struct.unpack_from("<7I", proof, 24)
    W, ce = SHAPE[air]
    assert W == width
    m = ext + 1
    log_N, log_f = log_n + blowup.bit_length() - 1, fold.bit_length() - 1
    nl = struct.unpack_from("<I", proof, 116)[0]
    L = {"air": air, "W": W, "ce": ce, "nq": nq, "m": m, "fold": fold, "log_N": log_N, "n_layers": nl, "rem_commit": 120 + 32 * nl}
    o = 152 + 32 * nl
    L["ood"] = o; o += 8 * (2 * W + ce) * m
    L["nonce"] = o; o += 8
    L["trace_rows"] = o; o += 8 * nq * W
    L["trace_paths"] = o; o += 32 * nq * log_N
    L["cons_rows"] = o; o += 8 * nq * ce * m
    L["cons_paths"] = o; o += 32 * nq * log_N
    L["layers"] = []
    lg = log_N
    for _ in range(nl):
        npos = struct.unpack_from("<I", proof, o)[0]
        depth = lg - log_f
        lay = {"count": o, "npos": npos, "rows": o + 4, "row_bytes": 8 * fold * m, "depth": depth}
        lay["paths"] = lay["rows"] + npos * lay["row_bytes"]
        o = lay["paths"] + 32 * depth * npos
        L["layers"].append(lay)
        lg = depth
    L["rem_len"] = struct.unpack_from("<I", proof, o)[0]
    L["remainder"] = o + 4
    assert L["remainder"] + 8 * L["rem_len"] * m == len(proof)
    return L


def element_sections(proof):
    """name -> (byte offset, words) of every section of field elements"""
    L = layout(proof)
    W, ce, m, nq = L["W"], L["ce"], L["m"], L["nq"]
    secs = {"ood_cur": (L["ood"], W * m), "ood_next": (L["ood"] + 8 * W * m, W * m), "ood_comp": (L["ood"] + 16 * W * m, ce * m),
            "trace_rows": (L["trace_rows"], nq * W), "cons_rows": (L["cons_rows"], nq * ce * m)}
    for l, lay in enumerate(L["layers"]):
        secs["layer%d_rows" % l] = (lay["rows"], lay["npos"] * L["fold"] * m)
    secs["remainder"] = (L["remainder"], L["rem_len"] * m)
    return secs


def tamper_offsets(proof):
    """name -> one byte offset inside every section of the proof: roots, both out-of-domain halves, nonce, trace / composition rows and
    paths, every layer's root, rows and paths, remainder commitment, remainder"""
    L = layout(proof)
    offs = {"trace_root": 53, "cons_root": 90, "rem_commit": L["rem_commit"] + 5, "nonce": L["nonce"] + 1,
            "trace_path": L["trace_paths"] + 32 * (L["log_N"] * (L["nq"] // 2) + 5) + 7,
            "cons_path": L["cons_paths"] + 32 * (L["log_N"] * (L["nq"] - 1) + 2) + 9}
    for name, (off, words) in element_sections(proof).items():
        offs[name] = off + 8 * (words // 2) + 2
    for l, lay in enumerate(L["layers"]):
        offs["layer%d_root" % l] = 120 + 32 * l + 17
        if lay["depth"]:
            offs["layer%d_path" % l] = lay["paths"] + 32 * lay["depth"] * (lay["npos"] // 2) + 4
    return offs


def words_canonical(proof):
    try:
        secs = element_sections(proof)
    except (AssertionError, KeyError, struct.error):
        return True   # the layout decides first
    return all(np.all(np.frombuffer(proof, np.uint64, n, off) < P) for off, n in secs.values() if n)


def noncanonical(proof, section):
    """a word >= p (p itself) in the middle of a field-element section"""
    off, words = element_sections(proof)[section]
    o = off + 8 * (words // 2)
    return proof[:o] + struct.pack("<Q", P) + proof[o + 8:]
