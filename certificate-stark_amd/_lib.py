"""ctypes binding of the C ABI declared in include/cstark.h (libcstark_hip.so).

The library is the product; there is no CPU fallback.  Loading fails loudly when the shared object
has not been built, and every compute call fails with CSTARK_ERR_NO_DEVICE when no GPU is visible.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSTARK_LIB") or os.path.join(HERE, "libcstark_hip.so")  # CSTARK_LIB: tuning variants

TX_TRACE_WIDTH, TX_CYCLE_LENGTH, TX_NUM_CONSTRAINTS, TX_NUM_PERIODIC = 94, 1024, 115, 48

u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)


class CstarkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("cstark error %d: %s" % (code, msg))
        self.code = code


class TxWitnessStruct(C.Structure):
    _fields_ = [("n_tx", C.c_uint32), ("merkle_depth", C.c_uint32),
                ("initial_roots", u64p), ("final_root", u64p), ("s_old_values", u64p), ("r_old_values", u64p),
                ("s_indices", u64p), ("r_indices", u64p), ("s_paths", u64p), ("r_paths", u64p),
                ("deltas", u64p), ("sig_rx", u64p), ("sig_s", u8p)]


class TxCoeffsStruct(C.Structure):
    _fields_ = [("t_alpha", C.c_uint64 * TX_NUM_CONSTRAINTS), ("t_beta", C.c_uint64 * TX_NUM_CONSTRAINTS),
                ("b_alpha", C.c_uint64 * 4), ("b_beta", C.c_uint64 * 4)]


class OptionsStruct(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("num_queries", "blowup_factor", "grinding_factor", "hash_fn",
                                           "field_extension", "fri_folding_factor", "fri_max_remainder")]


class SchnorrStatementStruct(C.Structure):
    _fields_ = [("n_sig", C.c_uint32), ("messages", u64p), ("sig_rx", u64p), ("sig_s", u8p)]


class TraceReportStruct(C.Structure):
    _fields_ = [("step", C.c_int64), ("constraint", C.c_uint32), ("bad_cycles", C.c_uint32), ("boundary", C.c_int32),
                ("boundary_register", C.c_uint32), ("boundary_step", C.c_uint64)]


class LedgerAuditReportStruct(C.Structure):
    _fields_ = [("consistent", C.c_uint32), ("n_bad", C.c_uint32), ("first_kind", C.c_uint32), ("first_level", C.c_uint32),
                ("first_index", C.c_uint64), ("n_nodes", C.c_uint64), ("slots_live", C.c_uint64), ("slots_held", C.c_uint64),
                ("slots_free", C.c_uint64)]


class LedgerSelectionStruct(C.Structure):
    _fields_ = [("n_candidates", C.c_uint32), ("n_selected", C.c_uint32), ("n_sig_checked", C.c_uint32), ("n_chunks", C.c_uint32),
                ("counts", C.c_uint32 * 10), ("root_after", C.c_uint64 * 7)]


class WitnessReportStruct(C.Structure):
    _fields_ = [("n_tx", C.c_uint32), ("merkle_depth", C.c_uint32), ("first_bad", C.c_int32), ("first_verdict", C.c_uint32),
                ("n_bad", C.c_uint32), ("reserved", C.c_uint32), ("final_root", C.c_uint64 * 7)]


WITNESS_CHECK_SIGNATURES = 1   # CSTARK_WITNESS_CHECK_SIGNATURES

TRACE_CLEAN = 0xFFFFFFFF
AIR_CYCLE_NAMES = ("transfer", "transfer", "signature", "trace", "link")   # per cstark_air_id: what one cycle of the trace is


def air_trace_shape(air, log_n):
    """cstark_air_trace_shape: (trace width, transition constraints, rows per cycle) of `air` at 2^log_n rows"""
    w, nc, lc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(load().cstark_air_trace_shape(C.c_int(air), C.c_uint32(log_n), C.byref(w), C.byref(nc), C.byref(lc)))
    return w.value, nc.value, 1 << lc.value


_lib = None


def _declare_convert(lib):
    """prototypes of the convert calls (include/cstark.h): their verify call's arguments, then form, out, capacities, out_lens,
    verdicts.  A CSTARK_LIB library built before the calls existed loads without them; calling one then fails by name."""
    if not hasattr(lib, "cstark_tx_convert"):
        return
    u8pp, sizes, i32p = C.POINTER(u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)
    options, tail = C.POINTER(OptionsStruct), [C.c_uint32, u8pp, sizes, sizes, i32p]
    lib.cstark_proof_convert_bound.argtypes = [u8p, C.c_size_t, C.c_uint32, sizes]
    lib.cstark_tx_convert.argtypes = [C.c_void_p, C.c_uint32, u8pp, sizes, u64p, u64p, options] + tail
    lib.cstark_air_convert.argtypes = [C.c_void_p, C.c_uint32, u8pp, sizes, i32p, u64p, options] + tail
    lib.cstark_schnorr_convert.argtypes = [C.c_void_p, C.c_uint32, u8pp, sizes, C.POINTER(SchnorrStatementStruct), options] + tail
    for fn in (lib.cstark_proof_convert_bound, lib.cstark_tx_convert, lib.cstark_air_convert, lib.cstark_schnorr_convert):
        fn.restype = C.c_int


def load():
    """Returns the loaded library; raises if it has not been built (python -m certificate_stark_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CstarkError(-2, "libcstark_hip.so is missing at %s: build it with __graft_entry__.build() "
                                  "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        # torch first: its wheel bundles its own HIP runtime, and the process must end up with ONE libamdhip64 -- if this
        # library pulled in the system copy before torch loaded, device discovery fails later ("no HIP device visible")
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        lib.cstark_last_error.restype = C.c_char_p
        lib.cstark_version.restype = C.c_char_p
        _declare_convert(lib)
        _lib = lib
    return _lib


_dbg = None


def load_debug():
    """The test-only companion library (include/cstark_debug.h): element-wise field / tower operations and micro-benchmarks."""
    global _dbg
    if _dbg is None:
        load()
        path = os.path.join(HERE, "libcstark_debug.so")
        if not os.path.exists(path):
            raise CstarkError(-2, "libcstark_debug.so is missing at %s: build it with __graft_entry__.build()" % path)
        _dbg = C.CDLL(path)
    return _dbg


def check(rc):
    if rc != 0:
        raise CstarkError(rc, load().cstark_last_error().decode())
