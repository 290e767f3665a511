"""Shared by test_gpu_commit_layouts.py, test_gpu_open_gather.py and test_open_reference_cpu.py: the plain references of the
commitment layouts and the openings -- the block order of a table's cosets, rows and authentication paths by indexing, the fold of a
path, the siblings a rank's own subtree supplies -- and the ctypes plumbing of include/cstark_debug_commit.h.

Layouts.  A table is [b][width][n] words, coset-major; leaf b j + k of its tree is the digest of row j of coset k; a node array is
[2 L][32] bytes with the root at 1 and the leaves at [L, 2 L).  BLOCK ORDER (csrc/blake3.h) with s = 2^log_s blocks of ce = b / s cosets:
coset k sits in slot (k mod s) ce + k // s.  Nothing here imports the product's own helpers."""
import ctypes as C

import numpy as np

P = 2**62 + 2**56 + 2**55 + 1
R_MOD_P = 2**64 % P
FILL = 0xA5
# memory-form words at the ends of the field and of the Montgomery form, with their neighbours (all below p)
EXTREME_WORDS = [0, 1, 2, P - 2, P - 1, R_MOD_P - 1, R_MOD_P, R_MOD_P + 1, (P - 1) // 2, (P + 1) // 2, 2**62, 2**62 - 1, 2**32 - 1, 2**32]
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1


# ---- block order ----------------------------------------------------------------------------------------------------------------------------
def coset_slot(k, log_b, log_s):
    s, ce = 1 << log_s, 1 << (log_b - log_s)
    return (k % s) * ce + k // s


def slot_coset(slot, log_b, log_s):
    s, ce = 1 << log_s, 1 << (log_b - log_s)
    return (slot % ce) * s + slot // ce


def to_slots(table, log_s):
    """natural table [b][width][n] -> the same cosets in block order"""
    b = table.shape[0]
    log_b = b.bit_length() - 1
    out = np.empty_like(table)
    for k in range(b):
        out[coset_slot(k, log_b, log_s)] = table[k]
    return out


# ---- openings by indexing ---------------------------------------------------------------------------------------------------------------------
def rows_at(table, positions, log_s=0):
    """table: what the kernel reads (slots); position b j + k -> row j of coset k, [count][width]"""
    b = table.shape[0]
    log_b = b.bit_length() - 1
    return np.array([table[coset_slot(p % b, log_b, log_s), :, p // b] for p in positions], np.uint64).reshape(len(positions), table.shape[1])


def path_at(nodes, pos, lvl0=0):
    """siblings of leaf pos from level lvl0 up to the children of the root: [log_leaves - lvl0][32]"""
    L = nodes.shape[0] // 2
    return [nodes[((L + pos) >> lvl) ^ 1] for lvl in range(lvl0, L.bit_length() - 1)]


def merge(left, right, hash_fn, oracle):
    """the parent of two digests, as oracle.merkle_build computes it: the root of the two-leaf tree"""
    return oracle.merkle_build(np.stack([left, right]), hash_fn)[1]


def fold_path(digest, pos, path, hash_fn, oracle):
    """a leaf digest folded up its path -> the root it implies"""
    for lvl, sib in enumerate(path):
        digest = merge(sib, digest, hash_fn, oracle) if (pos >> lvl) & 1 else merge(digest, sib, hash_fn, oracle)
    return digest


def window_siblings(nodes, pos, k0, nk, log_b=3):
    """What the owner of cosets [k0, k0 + nk) adds to the opening of global leaf pos = b j + k: the bottom log2(nk) levels of the path in
    the GLOBAL node array (its nk leaves of row j are a complete subtree of it), as 4 words per level; None for a foreign coset."""
    b = 1 << log_b
    if not k0 <= pos % b < k0 + nk:
        return None
    log_nk = nk.bit_length() - 1
    sib = path_at(nodes, pos)[:log_nk]
    return np.concatenate([s.view(np.uint64) for s in sib]) if sib else np.zeros(0, np.uint64)


def steered_positions(N, b, rng, count):
    """`count` positions of a domain of N = b n points that no drawn list promises, in this order of preference: the last and the first
    point, a sibling pair 2 i, 2 i + 1, a duplicate of 2 i, the neighbours of the ends, every coset of one row, then random ones; the
    whole list in descending order (drawn lists are never sorted that way)"""
    i = int(rng.integers(1, N // 2 - 1))
    j = int(rng.integers(0, N // b))
    pos = [N - 1, 0, 2 * i, 2 * i + 1, 2 * i, 1, N - 2] + [b * j + k for k in range(b)]
    pos += [int(v) for v in rng.integers(0, N, size=max(count - len(pos), 0))]
    return sorted(pos[:count], reverse=True)


# ---- include/cstark_debug_commit.h ------------------------------------------------------------------------------------------------------------
class GatherJobStruct(C.Structure):
    """struct cstark_debug_gather_job"""
    _fields_ = [("paths", C.c_uint32), ("d_src", C.c_void_p), ("src_bytes", C.c_size_t),
                ("width", C.c_uint32), ("log_n", C.c_uint32), ("log_b", C.c_uint32), ("log_s", C.c_uint32),
                ("log_leaves", C.c_uint32), ("lvl0", C.c_uint32), ("positions", C.c_void_p), ("count", C.c_uint32), ("dcount", C.c_int64),
                ("d_out", C.c_void_p), ("out_bytes", C.c_size_t)]


class RbOpenStruct(C.Structure):
    """struct cstark_debug_rb_open"""
    _fields_ = [("d_lde", C.c_void_p), ("d_clde", C.c_void_p), ("d_layer", C.c_void_p),
                ("lde_words", C.c_size_t), ("clde_words", C.c_size_t), ("layer_words", C.c_size_t),
                ("d_tnodes", C.c_void_p), ("d_cnodes", C.c_void_p), ("d_lnodes", C.c_void_p),
                ("tnodes_bytes", C.c_size_t), ("cnodes_bytes", C.c_size_t), ("lnodes_bytes", C.c_size_t),
                ("pos", C.c_void_p), ("lpos", C.c_void_p), ("lcount", C.c_void_p), ("d_out", C.c_void_p), ("out_bytes", C.c_size_t),
                ("nq", C.c_uint32), ("batch", C.c_uint32), ("n_layers", C.c_uint32),
                ("slot", C.c_size_t), ("trows", C.c_size_t), ("tpaths", C.c_size_t), ("crows", C.c_size_t), ("cpaths", C.c_size_t),
                ("lrows", C.c_size_t), ("lpaths", C.c_size_t)]


def _nbytes(t):
    return t.numel() * t.element_size()


class CommitDev:
    """device buffers of a Backend's device as torch tensors, and the entry points of cstark_debug_commit.h on its context"""

    def __init__(self, backend):
        from certificate_stark_amd import _lib
        self.backend, self.lib = backend, _lib.load_debug()
        u32, vp, sz = C.c_uint32, C.c_void_p, C.c_size_t
        self.lib.cstark_debug_hash_rows_slots.argtypes = [vp, u32, vp, sz, vp, sz, u32, u32, u32, u32, u32, u32]
        self.lib.cstark_debug_commit_batch.argtypes = [vp, u32, vp, sz, vp, sz, u32, u32, u32, u32, sz]
        self.lib.cstark_debug_merkle_batch.argtypes = [vp, u32, vp, sz, u32, u32, sz]
        self.lib.cstark_debug_gather.argtypes = [vp, C.POINTER(GatherJobStruct), u32]
        self.lib.cstark_debug_range_open.argtypes = [vp, C.POINTER(RbOpenStruct)]

    def u64(self, a):
        """a numpy array of words -> a device tensor of the same shape"""
        a = np.ascontiguousarray(a, np.uint64)
        return self.backend.from_numpy_u64(a.reshape(-1)).reshape(a.shape)

    def u8(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).to(self.backend.device)

    def filled(self, nbytes):
        """an output buffer of nbytes bytes, every byte FILL"""
        import torch
        return torch.full((nbytes,), FILL, dtype=torch.uint8, device=self.backend.device)

    @staticmethod
    def bytes_of(t):
        return t.cpu().numpy().view(np.uint8).reshape(-1)

    # -- row hashes ------------------------------------------------------------------------------------------------------------------------
    def hash_rows_slots(self, hash_fn, table_t, leaves_t, width, log_n, log_b, log_s, k0, nk):
        return self.lib.cstark_debug_hash_rows_slots(self.backend.ctx, hash_fn, table_t.data_ptr(), table_t.numel(), leaves_t.data_ptr(), _nbytes(leaves_t),
                                                     width, log_n, log_b, log_s, k0, nk)

    def commit_batch(self, hash_fn, table_t, nodes_t, gw, log_n, log_b, batch, stride):
        return self.lib.cstark_debug_commit_batch(self.backend.ctx, hash_fn, table_t.data_ptr(), table_t.numel(), nodes_t.data_ptr(), _nbytes(nodes_t),
                                                  gw, log_n, log_b, batch, stride)

    def merkle_batch(self, hash_fn, nodes_t, log_leaves, batch, stride):
        return self.lib.cstark_debug_merkle_batch(self.backend.ctx, hash_fn, nodes_t.data_ptr(), _nbytes(nodes_t), log_leaves, batch, stride)

    # -- openings: jobs = dicts with src (tensor), positions (list), out (tensor), optionally dcount, and either the fields of a rows job
    # (width, log_n, log_b, log_s) or of a paths job (log_leaves, lvl0) --------------------------------------------------------------------
    def gather(self, jobs):
        arr = (GatherJobStruct * max(len(jobs), 1))()
        keep = []
        for g, j in zip(arr, jobs):
            pos = np.ascontiguousarray(j["positions"], np.uint32)
            keep.append(pos)
            g.paths = 1 if "log_leaves" in j else 0
            g.d_src, g.src_bytes = j["src"].data_ptr(), _nbytes(j["src"])
            for f in ("width", "log_n", "log_b", "log_s", "log_leaves", "lvl0"):
                setattr(g, f, j.get(f, 0))
            g.positions, g.count, g.dcount = (pos.ctypes.data if pos.size else None), pos.size, j.get("dcount", -1)
            g.d_out, g.out_bytes = j["out"].data_ptr(), _nbytes(j["out"])
        return self.lib.cstark_debug_gather(self.backend.ctx, arr, len(jobs))

    def range_open(self, lde, clde, layer, tnodes, cnodes, lnodes, pos, lpos, lcount, out, nq, batch, n_layers, slot, offsets):
        """tensors (layer, lnodes: None without a layer), host position arrays, offsets = (trows, tpaths, crows, cpaths, lrows, lpaths)"""
        s = RbOpenStruct()
        keep = [np.ascontiguousarray(a, np.uint32) if a is not None else None for a in (pos, lpos, lcount)]
        for name, t, unit in (("lde", lde, "words"), ("clde", clde, "words"), ("layer", layer, "words"), ("tnodes", tnodes, "bytes"),
                              ("cnodes", cnodes, "bytes"), ("lnodes", lnodes, "bytes")):
            setattr(s, "d_" + name, t.data_ptr() if t is not None else None)
            setattr(s, name + "_" + unit, 0 if t is None else t.numel() if unit == "words" else _nbytes(t))
        s.pos, s.lpos, s.lcount = [a.ctypes.data if a is not None else None for a in keep]
        s.d_out, s.out_bytes = out.data_ptr(), _nbytes(out)
        s.nq, s.batch, s.n_layers, s.slot = nq, batch, n_layers, slot
        s.trows, s.tpaths, s.crows, s.cpaths, s.lrows, s.lpaths = offsets
        return self.lib.cstark_debug_range_open(self.backend.ctx, C.byref(s))
