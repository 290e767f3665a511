"""Proofs by a prover that cheats -- builders shared by test_oracle_cheats.py (CPU) and test_gpu_verify_cheats.py (GPU).

Every builder runs the CPU prover (oracle/prover.py) with ONE step altered and everything after it honest, so that every commitment,
opening and fold of the proof is consistent and exactly one check of the verifier can reject it:

  invalid_trace      one trace cell + 1                                        -> only the out-of-domain equation (OOD)
  wrong_composition  merged constraint evaluations + 1 (one point / all)       -> OOD
  shifted_deep       DEEP evaluations + constant before layer 0 is committed   -> only the DEEP value against the layer-0 row (LAYER_FOLDING, layer 0)
  forged_ood         invalid trace, H_0(z^ce) solved to satisfy the equation   -> only the low-degree test (REMAINDER_DEGREE)
  layer_count        one opened row of a layer removed / duplicated            -> LAYER_COUNT of that layer
  perturbed_fold     one fold output + 1 before it is committed                -> LAYER_FOLDING of the next layer / REMAINDER_FOLDING
  chosen_positions   honest proof whose nonce was searched for an index edge   -> OK

and byte mutators (flip, noncanonical) for proofs with two faults.  Not a conftest: nothing here changes how tests are collected."""
import functools
import struct

import numpy as np

P = (1 << 62) + (1 << 56) + (1 << 55) + 1
W, CE = 94, 8

# 1 transaction, depth 3: 2^10 rows, the smallest trace of TransactionAir; m, the coin's hash and the folding factor all vary
CONFIGS = {
    "base-blake3": (8, 8, 0, 0, 0, 4, 128),
    "quadratic-sha3": (12, 8, 0, 1, 1, 8, 128),
    "cubic-blake3": (16, 8, 0, 0, 2, 16, 256),
}
# cells of distinct constraint families (column, row); never row 0 or the last row, which public() reads the statement from
CELLS = {"rescue-register": (3, 5), "root-copy": (60, 100), "value": (70, 200), "range": (90, 300), "schnorr-phase": (10, 600)}


def witness(n_tx=1, depth=3, seed=0x5EED):
    from oracle import oracle as O
    return O.TxWitness.generate(n_tx, depth, seed=seed)


def _one():
    from oracle import verifier as V
    return V.to_mont(1)


def _add(a, v, sel=slice(None)):
    """a copy of the memory-form array a with the memory-form value v added (mod p) at flat index / slice sel"""
    b = np.array(a, np.uint64, copy=True)
    flat = b.reshape(-1)
    if isinstance(sel, int):
        sel = slice(sel, sel + 1)
    x = np.atleast_1d(flat[sel]).astype(object) + int(v)
    flat[sel] = np.array([int(e) % P for e in x], np.uint64)
    return b


class _Patched:
    """O.<name> replaced for the duration of one prove call"""

    def __init__(self, name, wrap):
        from oracle import oracle as O
        self.O, self.name, self.real = O, name, getattr(O, name)
        self.calls = 0
        real = self.real

        def f(*a, **k):
            out = wrap(self.calls, real(*a, **k))
            self.calls += 1
            return out
        self.f = f

    def __enter__(self):
        setattr(self.O, self.name, self.f)
        return self

    def __exit__(self, *exc):
        setattr(self.O, self.name, self.real)


def honest(w, options, **kw):
    from oracle import prover as OP
    return OP.prove(w, tuple(options), **kw)


# ---- an invalid trace, honestly committed -------------------------------------------------------------------------------------------
def _invalid_job(w, col, row):
    from oracle import oracle as O
    from oracle import prover as OP

    class Job(OP.TxJob):
        def build(self):
            trace = O.tx_build_trace(self.w)
            n = trace.shape[1]
            assert 0 < row < n - 1, "rows 0 and n - 1 carry the statement"
            trace[col, row] = (int(trace[col, row]) + _one()) % P
            assert O.tx_check_trace(trace, self.w.n_tx, self.w.depth) >= 0, "the altered cell is not constrained"
            return trace
    return Job(w)


def invalid_trace(w, options, col, row):
    return honest(w, options, job=_invalid_job(w, col, row))


def wrong_composition(w, options, every_point=False):
    """the merged constraint evaluations (job.combine) + 1 at one point of the constraint-evaluation domain, or at every point, before
    they are interpolated into the composition columns"""
    from oracle import prover as OP

    class Job(OP.TxJob):
        def combine(self, *a, **k):
            out = OP.TxJob.combine(self, *a, **k)
            return _add(out, _one()) if every_point else _add(out, _one(), 3 * out.shape[1] + 77)
    return honest(w, options, job=Job(w))


def shifted_deep(w, options, component=0, shift=None):
    """every DEEP evaluation + a constant (in one component of the extension) before layer 0 is committed: still of low degree"""
    m = options[4] + 1
    assert 0 <= component < m
    shift = _one() if shift is None else shift

    def wrap(call, out):
        if m == 1:
            return _add(out, shift)
        out = np.array(out, np.uint64, copy=True)     # [m][b][n]
        out[component] = _add(out[component], shift)
        return out
    with _Patched("deep_composition_ext" if m > 1 else "deep_composition", wrap) as pt:
        proof = honest(w, options)
    assert pt.calls == 1
    return proof


def forged_ood(w, options, col, row):
    """Pass 1: invalid_trace; the restated verifier gives z and both sides of the out-of-domain equation.  Pass 2: the same proof with
    lhs - rhs added to H_0(z^ce), which the equation then accepts (z and the constraint coefficients do not depend on the out-of-domain
    values).  H_0's opened values no longer interpolate through the forged one, so the DEEP quotient is not a polynomial."""
    from oracle import verifier as V
    m = options[4] + 1
    first = invalid_trace(w, options, col, row)
    probe = {}
    try:
        V.verify(first, w.initial_roots[0], w.final_root, probe=probe)
        raise AssertionError("the invalid trace was accepted")
    except V.VerifierError as e:
        assert "out-of-domain" in str(e)
    if m == 1:
        delta = [(probe["ood_lhs"] - probe["ood_rhs"]) % P]
    else:
        delta = list(V.e_sub(probe["ood_lhs"], probe["ood_rhs"]))
    delta = [V.to_mont(v) for v in delta]

    if m == 1:
        def wrap(call, out):    # calls: the trace frame, then the composition columns at z^ce: [1][ce]
            return _add(out, delta[0], 0) if call == 1 else out
        name, calls = "evaluate_polys_at", 2
    else:
        def wrap(call, out):    # calls: frame at z, at z w, then [m ce][m]: row m i + k = component polynomial k of H_i; H_0 += delta
            if call != 2:
                return out
            for q in range(m):
                out = _add(out, delta[q], q)
            return out
        name, calls = "evaluate_polys_at_ext", 3
    with _Patched(name, wrap) as pt:
        proof = honest(w, options, job=_invalid_job(w, col, row))
    assert pt.calls == calls
    return proof


def perturbed_fold(w, options, call, idx=None):
    """the `call`-th fold output (0 = layer 1; n_layers - 1 = the remainder) + 1 before it is committed (everywhere, or at idx)"""
    def wrap(c, out):
        if c != call:
            return out
        return _add(out, _one()) if idx is None else _add(out, _one(), idx)
    with _Patched("fri_fold_ext" if options[4] else "fri_fold", wrap):
        return honest(w, options)


# ---- chosen query positions ---------------------------------------------------------------------------------------------------------
def _domain(options, log_n=10):
    return (1 << log_n) * options[1]


WANTS = ("first", "last", "repeat", "same-row")


def chosen_positions(w, options, want, log_n=10):
    """An honest proof (grinding 0) whose nonce was searched until the query positions contain an index edge:
      first     position 0                       last      position N - 1
      repeat    the coin draws a position twice (query positions are distinct by convention: the repeat is skipped, which is the edge)
      same-row  two positions in the same layer-0 row
    Returns (proof, q): q = the index of the query at the edge (for repeat / same-row: the later of the two)."""
    N, fold = _domain(options, log_n), options[5]
    rows = N // fold
    found = {}

    def choose(pos, draws):
        if want == "first" and 0 in pos:
            found["q"] = pos.index(0)
        elif want == "last" and N - 1 in pos:
            found["q"] = pos.index(N - 1)
        elif want == "repeat" and len(draws) > len(pos):
            rep = [v for i, v in enumerate(draws) if v in draws[:i]][0]
            found["q"] = pos.index(rep)
        elif want == "same-row":
            r = [p & (rows - 1) for p in pos]
            dup = [i for i, v in enumerate(r) if v in r[:i]]
            if dup:
                found["q"] = dup[0]
        return "q" in found
    assert want in WANTS
    proof = honest(w, options, choose_nonce=choose)
    return proof, found["q"]


# ---- bytes --------------------------------------------------------------------------------------------------------------------------
def layout(proof):
    """section offsets of a TransactionAir proof (layout of include/cstark.h), from its header and count words"""
    log_n = struct.unpack_from("<I", proof, 16)[0]
    nq, blowup, _, _, ext, fold, _ = struct.unpack_from("<7I", proof, 24)
    m = ext + 1
    log_N, log_f = log_n + blowup.bit_length() - 1, fold.bit_length() - 1
    nl = struct.unpack_from("<I", proof, 116)[0]
    L = {"nq": nq, "m": m, "fold": fold, "log_N": log_N, "n_layers": nl, "rem_commit": 120 + 32 * nl}
    o = 152 + 32 * nl
    L["ood"] = o; o += 8 * (2 * W + CE) * m
    L["nonce"] = o; o += 8
    L["trace_rows"] = o; o += 8 * nq * W
    L["trace_paths"] = o; o += 32 * nq * log_N
    L["cons_rows"] = o; o += 8 * nq * CE * m
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


def layer_count(proof, layer, delta):
    """the last opened row of a layer and its path removed (delta = -1) or repeated (+1), the count word adjusted: the result parses"""
    L = layout(proof)
    lay = L["layers"][layer]
    npos, rb, pb = lay["npos"], lay["row_bytes"], 32 * lay["depth"]
    rows = proof[lay["rows"]:lay["paths"]]
    paths = proof[lay["paths"]:lay["paths"] + npos * pb]
    if delta == -1:
        assert npos >= 2
        rows, paths = rows[:-rb], paths[:-pb] if pb else paths
    else:
        assert delta == 1 and npos < L["nq"], "a count above num_queries is a layout error"
        rows, paths = rows + rows[-rb:], paths + (paths[-pb:] if pb else b"")
    out = proof[:lay["count"]] + struct.pack("<I", npos + delta) + rows + paths + proof[lay["paths"] + npos * pb:]
    layout(out)
    return out


def can_grow(proof, layer):
    L = layout(proof)
    return L["layers"][layer]["npos"] < L["nq"]


def flip_at(proof, off, bit=0x01):
    b = bytearray(proof)
    b[off] ^= bit
    return bytes(b)


def flip(proof, name, bit=0x01):
    """one byte of a named section (the offsets of test_gpu_verify._tamper_offsets)"""
    from test_gpu_verify import _tamper_offsets
    return flip_at(proof, _tamper_offsets(proof)[name], bit)


def _section_word(proof, section, word=0):
    """byte offset of a field-element word: section = ood | trace_row | cons_row | layer<l> | remainder"""
    L = layout(proof)
    if section.startswith("layer"):
        base = L["layers"][int(section[5:])]["rows"]
    else:
        base = L[{"ood": "ood", "trace_row": "trace_rows", "cons_row": "cons_rows", "remainder": "remainder"}[section]]
    return base + 8 * word


def noncanonical(proof, section, word=0):
    """a word >= p (here p itself) in a field-element section"""
    o = _section_word(proof, section, word)
    return proof[:o] + struct.pack("<Q", P) + proof[o + 8:]


def query_replay(proof, r0, r1):
    """(positions, draws) of a proof that passes every check up to the proof of work, from the restated verifier's replay: the query
    positions, and every integer the coin produced for them (longer than the positions when a repeat was skipped)"""
    from oracle import verifier as V
    probe = {}
    try:
        V.verify(proof, r0, r1, probe=probe)
    except V.VerifierError:
        pass
    return probe["positions"], probe["draws"]


def query_positions(proof, r0, r1):
    return query_replay(proof, r0, r1)[0]


# ---- the cases both halves of the suite use -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def isolating_cases(cfg):
    """name -> (proof, the one verdict that must reject it, a part of the restated verifier's message) for one of CONFIGS, with the
    honest proof under "honest".  Built once per process."""
    w, o = witness(), CONFIGS[cfg]
    m = o[4] + 1
    cases = {"honest": (honest(w, o), "OK", "")}
    for name, (col, row) in CELLS.items():
        cases["invalid_trace:" + name] = (invalid_trace(w, o, col, row), "OOD", "out-of-domain")
    cases["wrong_composition:one-point"] = (wrong_composition(w, o), "OOD", "out-of-domain")
    cases["wrong_composition:every-point"] = (wrong_composition(w, o, every_point=True), "OOD", "out-of-domain")
    for k in range(m):
        cases["shifted_deep:component-%d" % k] = (shifted_deep(w, o, k), "LAYER_FOLDING", "layer 0: evaluation differs")
    for name in ("value", "rescue-register"):
        cases["forged_ood:" + name] = (forged_ood(w, o, *CELLS[name]), "REMAINDER_DEGREE", "low-degree")
    proof = cases["honest"][0]
    nl = layout(proof)["n_layers"]
    # the folds of test_gpu_verify_fri.py at this size: layer 1 and the remainder altered before they are committed
    cases["perturbed_fold:layer-1"] = (perturbed_fold(w, o, 0), "LAYER_FOLDING", "layer 1: evaluation differs")
    cases["perturbed_fold:remainder"] = (perturbed_fold(w, o, nl - 1), "REMAINDER_FOLDING", "remainder differs")
    for layer in sorted({0, nl // 2, nl - 1}):   # the first, a middle and the last layer
        cases["layer_count:%d:-1" % layer] = (layer_count(proof, layer, -1), "LAYER_COUNT", "layer %d: wrong number" % layer)
        if can_grow(proof, layer):
            cases["layer_count:%d:+1" % layer] = (layer_count(proof, layer, +1), "LAYER_COUNT", "layer %d: wrong number" % layer)
    return cases


@functools.lru_cache(maxsize=None)
def edge_cases(cfg):
    """want -> (proof, index of the query at the edge) for one of CONFIGS"""
    w, o = witness(), CONFIGS[cfg]
    return {want: chosen_positions(w, o, want) for want in WANTS}
