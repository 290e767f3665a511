"""SchnorrAir proofs by a prover that cheats -- builders shared by test_oracle_schnorr_cheats.py (CPU) and test_gpu_schnorr_verify.py
(GPU), in the manner of cheating_sub_airs.py: the CPU prover (oracle/prover.py, SchnorrJob) with ONE step altered and everything after it
honest.  A statement here is an oracle.SchnorrWitness (messages [n][28], sig_rx [n][6], sig_s [n][32]: all of it is public).

  invalid_trace     one trace cell + 1, honestly committed                          -> only the out-of-domain equation (OOD)
  lying_statement   public() states one word more than the trace was built from; the channel is seeded with the lie and the proof is
                    verified against it.  Three words, one per kind of value the verifier forms from the statement:
                      "rx"    R.x[0][0]: a sequence-assertion value                 -> the boundary terms (OOD)
                      "pkey"  message word 3, a public-key word: a block-constant public-input column     -> the transition terms (OOD)
                      "msg"   message word 20: a hash-input column, non-zero on four rows of the block    -> the transition terms (OOD)
  shifted_deep      DEEP evaluations + 1 before they are committed                  -> LAYER_FOLDING at layer 0

Not a conftest: nothing here changes how tests are collected."""
import copy
import functools

import numpy as np

from cheating_prover import P, _Patched, _add, _one

SCHNORR = 2
OPTIONS = (8, 8, 0, 0, 0, 4, 128)   # 1 signature: 2^9 rows, the smallest trace; one FRI layer
# one cell (column, row) per register group: a point register of s*G, a limb accumulator of h, the hash state (rows 8 i + 7 take a message
# chunk, the others a Rescue round).  Never a row = 0 or 511 mod 512: the assertions read those.
CELLS = {"point": (3, 100), "limb": (39, 200), "hash": (45, 10)}
LIES = {"rx": ("sig_rx", 0, 0), "pkey": ("messages", 0, 3), "msg": ("messages", 0, 20)}


def witness(n_sig=1, seed=0x5EED):
    from oracle import oracle as O
    return O.SchnorrWitness.generate(n_sig, seed=seed)


def changed(w, field, t, k, delta=None):
    """a copy of the statement with word [t][k] of `field` + 1 (a field element in memory form), or byte [t][k] of sig_s flipped"""
    c = copy.copy(w)
    c.messages, c.sig_rx, c.sig_s = w.messages.copy(), w.sig_rx.copy(), w.sig_s.copy()
    a = getattr(c, field)
    if field == "sig_s":
        a[t, k] ^= 0x01
    else:
        a[t, k] = (int(a[t, k]) + (_one() if delta is None else delta)) % P
    return c


def prove(job, options):
    from oracle import prover as OP
    return OP._prove_job(job, tuple(options))


def honest(n_sig=1, options=OPTIONS, seed=0x5EED):
    from oracle import prover as OP
    w = witness(n_sig, seed)
    return prove(OP.SchnorrJob(w), options), w


def verify(proof, w, options=None):
    from oracle import verifier as V
    return V.verify_schnorr(proof, w, options=options)


def oracle_verdict(proof, w, options=None):
    """the restated verifier's reason as a verdict name: the message table of test_gpu_verify.oracle_verdict, extended by SchnorrAir's
    two messages"""
    from oracle import verifier as Vf
    try:
        verify(proof, w, options)
        return "OK"
    except Vf.VerifierError as e:
        msg = str(e)
    table = [("not a SchnorrAir proof", "UNSUPPORTED"), ("different number of signatures", "OOD"), ("proof options differ", "OPTIONS_MISMATCH"),
             ("out-of-domain", "OOD"), ("proof of work", "POW"), ("trace opening", "TRACE_OPENING"), ("composition opening", "COMPOSITION_OPENING"),
             ("wrong number", "LAYER_COUNT"), ("opening does not match", "LAYER_OPENING"), ("evaluation differs", "LAYER_FOLDING"),
             ("remainder differs", "REMAINDER_FOLDING"), ("low-degree", "REMAINDER_DEGREE")]
    if msg.startswith("remainder does not match its commitment"):
        return "REMAINDER_COMMITMENT"
    for key, name in table:
        if key in msg:
            return name
    return "MALFORMED"


# ---- the three deviations -------------------------------------------------------------------------------------------------------------
def invalid_trace(col, row, n_sig=1, options=OPTIONS):
    from oracle import prover as OP

    class Job(OP.SchnorrJob):
        def build(self):
            trace = OP.SchnorrJob.build(self)
            assert row % 512 not in (0, 511), "rows 0 and 511 of a block carry the assertions"
            trace[col, row] = (int(trace[col, row]) + _one()) % P
            return trace
    w = witness(n_sig)
    return prove(Job(w), options), w


def lying_statement(which, n_sig=1, options=OPTIONS):
    """returns the proof and the statement it was seeded with (the lie); the trace, the public-input columns and the sequence
    polynomials of the constraint evaluations are those of the true witness"""
    from oracle import prover as OP
    w = witness(n_sig)
    lie = changed(w, *LIES[which])

    class Job(OP.SchnorrJob):
        def public(self, trace):
            return [int(v) for v in lie.messages.reshape(-1)] + [int(v) for v in lie.sig_rx.reshape(-1)], lie.sig_s.tobytes()
    return prove(Job(w), options), lie


def shifted_deep(n_sig=1, options=OPTIONS, component=0):
    from oracle import prover as OP
    m = options[4] + 1

    def wrap(call, out):
        if m == 1:
            return _add(out, _one())
        out = np.array(out, np.uint64, copy=True)
        out[component] = _add(out[component], _one())
        return out
    w = witness(n_sig)
    with _Patched("deep_composition_ext" if m > 1 else "deep_composition", wrap) as pt:
        proof = prove(OP.SchnorrJob(w), options)
    assert pt.calls == 1
    return proof, w


@functools.lru_cache(maxsize=None)
def isolating_cases():
    """name -> (proof, statement, the one verdict that rejects it, a part of the restated verifier's message)"""
    cases = {}
    for name, (col, row) in CELLS.items():
        cases["invalid_trace:" + name] = (*invalid_trace(col, row), "OOD", "out-of-domain")
    for which in LIES:
        cases["lying_statement:" + which] = (*lying_statement(which), "OOD", "out-of-domain")
    cases["lying_statement:pkey:2-signatures-cubic"] = (*lying_statement("pkey", 2, (8, 8, 0, 1, 2, 8, 128)), "OOD", "out-of-domain")
    cases["shifted_deep"] = (*shifted_deep(), "LAYER_FOLDING", "layer 0: evaluation differs")
    return cases
