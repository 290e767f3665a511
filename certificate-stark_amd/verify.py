"""Verification surfaces that need no GPU: the verdict names of include/cstark.h, VerifierError, inspect_proof (the host parser) and
convert_bound (the capacity of a proof in the other form).

The verifier itself is Backend.tx_verify / TransactionExample.verify (cstark_tx_verify on the GPU)."""
import ctypes as C

from . import _lib

# cstark_verdict, in enum order (the value is only a name; the order in which checks fail is documented in include/cstark.h)
VERDICTS = ("OK", "MALFORMED", "UNSUPPORTED", "OPTIONS_MISMATCH", "OOD", "REMAINDER_COMMITMENT", "POW", "TRACE_OPENING",
            "COMPOSITION_OPENING", "LAYER_COUNT", "LAYER_OPENING", "LAYER_FOLDING", "REMAINDER_FOLDING", "REMAINDER_DEGREE")
VERIFY_STAGES = ("host", "h2d", "transcript", "ood", "openings", "fri", "remainder_reduce_d2h")


class VerifierError(Exception):
    """A rejected proof: the counterpart of winterfell's Result<(), VerifierError>.  .verdict is the cstark_verdict value, .reason its
    name."""

    def __init__(self, verdict):
        self.verdict = int(verdict)
        self.reason = VERDICTS[self.verdict] if 0 <= self.verdict < len(VERDICTS) else "UNKNOWN_%d" % self.verdict
        super().__init__("proof rejected: %s" % self.reason)


class ProofInfoStruct(C.Structure):
    _fields_ = [("air", C.c_uint32), ("trace_width", C.c_uint32), ("log_n", C.c_uint32), ("header_word", C.c_uint32),
                ("options", _lib.OptionsStruct)]


class ProofInfo:
    """What cstark_proof_inspect reads from a proof: verdict (OK or MALFORMED), AIR id, trace width, log2 of the trace length, the
    header word (Merkle depth for TransactionAir) and the 7 option values [num_queries, blowup, grinding, hash_fn, extension, folding,
    max_remainder]."""

    def __init__(self, s, verdict):
        self.verdict = int(verdict)
        self.air, self.trace_width, self.log_n, self.header_word = int(s.air), int(s.trace_width), int(s.log_n), int(s.header_word)
        o = s.options
        self.options = [int(o.num_queries), int(o.blowup_factor), int(o.grinding_factor), int(o.hash_fn), int(o.field_extension),
                        int(o.fri_folding_factor), int(o.fri_max_remainder)]

    @property
    def depth(self):
        return self.header_word

    @property
    def ok(self):
        return self.verdict == 0


def proof_form(proof):
    """cstark_proof_form: "plain" or "compact" by the proof's magic (host only); ValueError when it has neither"""
    b = bytes(proof)
    buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
    form = C.c_uint32(0)
    if _lib.load().cstark_proof_form(buf, C.c_size_t(len(b)), C.byref(form)) != 0:
        raise ValueError("neither a plain nor a compact proof")
    return ("plain", "compact")[form.value]


def convert_bound(proof, form):
    """cstark_proof_convert_bound: a capacity that holds `proof` converted to `form` ("plain" or "compact"; 0 / 1 are accepted too)
    whatever its positions -- to "plain" the exact plain length, to "compact" the plain length plus 4 bytes per tree.  Host only;
    ValueError for another form or a proof whose layout does not parse."""
    b = bytes(proof)
    buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
    form = {"plain": 0, "compact": 1}.get(form, form)
    if form not in (0, 1):
        raise ValueError("form is 'plain' or 'compact', not %r" % (form,))
    bound = C.c_size_t(0)
    if _lib.load().cstark_proof_convert_bound(buf, C.c_size_t(len(b)), C.c_uint32(form), C.byref(bound)) != 0:
        raise ValueError("the proof's layout does not parse")
    return int(bound.value)


def inspect_proof(proof):
    """cstark_proof_inspect: the complete layout check of a proof of any of the five AIRs, in either form, on the host (no GPU, no context)."""
    b = bytes(proof)
    buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
    info, verdict = ProofInfoStruct(), C.c_int32(-1)
    _lib.check(_lib.load().cstark_proof_inspect(buf, C.c_size_t(len(b)), C.byref(info), C.byref(verdict)))
    return ProofInfo(info, verdict.value)
