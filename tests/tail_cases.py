"""Shared by test_gpu_channel_steps.py, test_gpu_fri_coin.py and test_gpu_pow_search.py: the Python side of the kernels that branch on
hash output -- the reference coin with a seed of the test's choice, candidate lists, steered constants and their searches -- and the
ctypes plumbing of include/cstark_debug_channel.h.

A steered constant is an index i: the 32 bytes are tagged(tag, i) = digest(tag || le64(i)).  search(tag, wanted) is the loop that
found it; every test re-derives the property it needs from the reference before it asks the GPU (require)."""
import ctypes as C
import struct

import numpy as np

P = 2**62 + 2**56 + 2**55 + 1
R = 2**64
R_INV = pow(R, -1, P)
NONE64 = 2**64 - 1
NON_ELEMENT = 0xFFFFFFFFFFFFFFFE            # no field element in either form: above p
NON_POSITION = 0xDEADBEEF                   # above every position of a domain of at most 2^31 points


def mont(x):
    return x * R % P


def canon(w):
    return int(w) * R_INV % P


def _O():
    from oracle import oracle as O
    return O


def _V():
    from oracle import verifier as V
    return V


def le64(v):
    return struct.pack("<Q", v)


def H(data, hash_fn=0):
    return _O().digest(data, hash_fn)


def tagged(tag, i, hash_fn=0):
    return H(tag.encode() + le64(i), hash_fn)


def search(tag, wanted, limit=1 << 22, hash_fn=0, start=0):
    """the smallest i >= start with wanted(tagged(tag, i)): how the literals in the tests were found"""
    for i in range(start, limit):
        if wanted(tagged(tag, i, hash_fn)):
            return i
    raise RuntimeError("no %s below %d" % (tag, limit))


def require(cond, what):
    """a steered constant that lost its property is an error of the test, not a finding about the kernel"""
    if not cond:
        raise RuntimeError("steered constant is wrong: " + what)


# ---- the reference coin -----------------------------------------------------------------------------------------------------------------
def first_counter():
    return _V().CONV["coin_first_counter"]


def coin_at(seed, hash_fn=0):
    """oracle/verifier.py's Coin standing at `seed` (32 bytes), nothing drawn yet"""
    V = _V()
    c = V.Coin(b"", hash_fn)
    c.seed, c.counter = bytes(seed), first_counter() - 1
    return c


def candidates(seed, n, hash_fn=0, start=None):
    """the 64-bit integers of counters start .. start + n - 1 (start: the coin's first counter)"""
    start = first_counter() if start is None else start
    return [struct.unpack("<Q", H(bytes(seed) + le64(start + k), hash_fn)[:8])[0] for k in range(n)]


def is_element(v):
    return v < P or not _V().CONV["coin_reject_above_p"]


def accepted_offsets(seed, n):
    """which of the first n counters yield a field element"""
    return [k for k, v in enumerate(candidates(seed, n)) if is_element(v)]


def elems_digest(words, hash_fn=0):
    """digest of a list of field elements (memory-form words) as the prover absorbs it"""
    return H(_V().elem_bytes(np.ascontiguousarray(words, np.uint64)), hash_fn)


def pow_value(seed, nonce, hash_fn=0):
    return struct.unpack("<Q", H(bytes(seed) + le64(nonce), hash_fn)[:8])[0]


def pow_scan(seed, base, count, bits, hash_fn=0):
    """the smallest nonce of [base, base + count) whose digest has `bits` low zero bits, or ~0"""
    mask = (1 << bits) - 1
    for nonce in range(base, base + count):
        if pow_value(seed, nonce, hash_fn) & mask == 0:
            return nonce
    return NONE64


def pow_sequential(seed, bits, hash_fn=0, limit=1 << 20):
    """the sequential search of oracle/prover.py: nonces 1, 2, ..."""
    got = pow_scan(seed, 1, limit, bits, hash_fn)
    if got == NONE64:
        raise RuntimeError("no nonce below %d" % limit)
    return got


# ---- device memory and include/cstark_debug_channel.h -------------------------------------------------------------------------------------
class ChanAbsorbStruct(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("count", C.c_uint32), ("ptr", C.c_void_p), ("value", C.c_uint64), ("copy_out", C.c_void_p)]


class ChanStepStruct(C.Structure):
    """struct cstark_debug_chan_step"""
    _fields_ = [("seed", C.c_void_p), ("init", C.c_uint32), ("prefix_len", C.c_uint32), ("npub", C.c_uint32), ("prefix", C.c_uint8 * 32),
                ("pub", C.c_void_p), ("absorb", ChanAbsorbStruct * 3),
                ("draw", C.c_uint32), ("count", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("stride", C.c_uint32), ("per", C.c_uint32),
                ("m", C.c_uint32), ("set_stride", C.c_uint32), ("out", C.c_void_p), ("out2", C.c_void_p), ("w", C.c_uint64),
                ("log_domain", C.c_uint32), ("log_f", C.c_uint32), ("n_layers", C.c_uint32), ("slot", C.c_uint32),
                ("pos", C.c_void_p), ("cnt", C.c_void_p)]


CHAN_DIGEST, CHAN_ELEMS, CHAN_INT = 1, 2, 3
DRAW_LINEAR, DRAW_COEFFS, DRAW_DEEP, DRAW_POINT, DRAW_QUERIES = 1, 2, 3, 4, 5
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1


class Dev:
    """device buffers of a Backend's device as torch tensors, and the debug entry points on its context"""

    def __init__(self, backend):
        from certificate_stark_amd import _lib
        self.backend, self.lib = backend, _lib.load_debug()
        self.lib.cstark_debug_channel_step.argtypes = [C.c_void_p, C.POINTER(ChanStepStruct)]
        self.lib.cstark_debug_fri_coin.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.cstark_debug_grind_chunk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
        self.lib.cstark_debug_grind_search.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]

    def u64(self, values):
        return self.backend.from_numpy_u64(np.ascontiguousarray(values, np.uint64).reshape(-1))

    def u32(self, values):
        import torch
        return torch.from_numpy(np.ascontiguousarray(values, np.uint32).reshape(-1).view(np.int32).copy()).to(self.backend.device)

    def raw(self, data):
        import torch
        return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(self.backend.device)

    @staticmethod
    def ptr(t):
        if t is None:
            return None
        assert t.is_contiguous()
        return t.data_ptr()

    @staticmethod
    def get_u64(t):
        return [int(v) for v in t.cpu().numpy().view(np.uint64)]

    @staticmethod
    def get_u32(t):
        return [int(v) for v in t.cpu().numpy().view(np.uint32)]

    @staticmethod
    def get_raw(t):
        return t.cpu().numpy().tobytes()

    # -- the channel: keyword arguments are the fields of ChanStepStruct; absorbs = [(kind, count, tensor, value, copy_out tensor)] --
    def channel_step(self, seed_t, absorbs=(), prefix=b"", pub=None, **fields):
        s = ChanStepStruct()
        s.seed, s.m = self.ptr(seed_t), 1
        s.prefix_len = len(prefix)
        for i, byte in enumerate(bytes(prefix)[:32]):
            s.prefix[i] = byte
        s.pub = self.ptr(pub)
        for k, (kind, count, t, value, copy_out) in enumerate(absorbs):
            s.absorb[k].kind, s.absorb[k].count, s.absorb[k].ptr, s.absorb[k].value, s.absorb[k].copy_out = kind, count, self.ptr(t), value, self.ptr(copy_out)
        for name, v in fields.items():
            assert name in dict(ChanStepStruct._fields_), name
            setattr(s, name, self.ptr(v) if name in ("out", "out2", "pos", "cnt") else v)
        return self.lib.cstark_debug_channel_step(self.backend.ctx, C.byref(s))

    def fri_coin(self, m, seed_t, root_t, alpha_t, root_out_t):
        return self.lib.cstark_debug_fri_coin(self.backend.ctx, m, self.ptr(seed_t), self.ptr(root_t), self.ptr(alpha_t), self.ptr(root_out_t))

    def grind_chunk(self, form, seeds, batch, base, count, bits, found_t):
        """form 0: seeds = 32 host bytes; 1 (Blake3), 2 (Sha3): seeds = a device tensor of batch seeds"""
        host = C.create_string_buffer(bytes(seeds), 32) if form == 0 else None   # (alive until the call returns)
        sp = C.cast(host, C.c_void_p) if form == 0 else self.ptr(seeds)
        return self.lib.cstark_debug_grind_chunk(self.backend.ctx, form, sp, batch, base, count, bits, self.ptr(found_t))

    def grind_search(self, seed, hash_fn, bits, chunk):
        found_t, nonce = self.u64([0] * 5), C.c_uint64(0)
        rc = self.lib.cstark_debug_grind_search(self.backend.ctx, self.ptr(found_t), bytes(seed), hash_fn, bits, chunk, C.byref(nonce))
        assert rc == 0, rc
        return nonce.value
