"""Shared by test_gpu_coset_transfer.py and test_coset_reference_cpu.py: what the vectors of the coset-transfer kernels MEAN, computed
with the oracle's transforms, and the ctypes plumbing of include/cstark_debug_coset.h.

Setting.  p = 2^62 + 2^56 + 2^55 + 1, g = 3 the LDE offset, w_m the oracle's root of unity of order m (w_8n^2 = w_4n, w_4n^4 = w_n),
W8 = w_8n^n.  A TABLE is a polynomial S(g y) = sum_t a_t y^t with 4n coefficients.  The 8n-point LDE domain is x = g w_8n^k w_n^j:
coset k, row j; the even cosets k = 2 kc are the 4n-point domain of y = w_4n^kc w_n^j, the odd ones k' = 2 kc + 1 are what the
extension reaches.  An INTERPOLANT of a coset is the inverse n-point transform of the values on it: B_kc on the even cosets (the
kernels' input); on an odd coset the kernels write the vector that, multiplied element-wise by w_8n^(k' q) and transformed, gives the
values there (the transform's prescale table supplies that twist in the product).

Every array here is numpy uint64 in memory form (Montgomery words: oracle.to_mont / oracle.from_mont at the edges), every power is
Python's pow on integers, every transform is oracle.ntt.  Nothing here imports the product's own helpers."""
import ctypes as C

import numpy as np

P = 2**62 + 2**56 + 2**55 + 1
G = 3
FILL = 0xA5
FILL_WORD = 0xA5A5A5A5A5A5A5A5
NOT_A_FIELD_ELEMENT = 0xFFFFFFFFFFFFFFFF
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1
MERGE_FAMILIES, MERGE_TERMS = 5, 4     # cs::COSET_MERGE_MAX_FAMILIES, cs::COSET_MERGE_MAX_TERMS


class Ref:
    """the references, over one oracle"""

    def __init__(self, oracle):
        self.O = oracle
        self._tables = {}

    # ---- integers <-> memory form ---------------------------------------------------------------------------------------------------
    def mont(self, ints):
        a = np.array([int(v) % P for v in np.asarray(ints, dtype=object).reshape(-1)], dtype=np.uint64)
        return self.O.to_mont(a).reshape(np.shape(ints))

    def ints(self, words):
        w = np.ascontiguousarray(words, np.uint64)
        return [int(v) for v in self.O.from_mont(w.reshape(-1))]

    def root(self, log_m):
        return int(self.O.from_mont([self.O.root_of_unity(log_m)])[0])

    def powers(self, base, count):
        """memory-form table of base^q, q < count (integer products)"""
        key = (base % P, count)
        if key not in self._tables:
            out, v = [], 1
            for _ in range(count):
                out.append(v)
                v = v * base % P
            self._tables[key] = self.mont(out)
        return self._tables[key]

    def scale(self, vec, base):
        """vec[q] base^q"""
        return self.O.fp_mul(vec, self.powers(base, vec.size))

    # ---- a table on the cosets ---------------------------------------------------------------------------------------------------------
    def even_interpolants(self, a):
        """coefficients a [4n] of S(g y) -> B [4][n]: B_kc = the inverse transform of S on y = w_4n^kc w_n^j (point 4 j + kc of <w_4n>)"""
        v = self.O.ntt(a)
        return np.stack([self.O.ntt(v[kc::4], inverse=True) for kc in range(4)])

    def even_interpolants_closed(self, a):
        """the same in closed form: B_k[q] = w_4n^(k q) sum_i a_(q + n i) w_4^(k i)"""
        a = self.ints(a)
        n = len(a) // 4
        w4n = self.root(n.bit_length() + 1)
        w4 = pow(w4n, n, P)
        return self.mont([[pow(w4n, k * q, P) * sum(a[q + n * i] * pow(w4, k * i, P) for i in range(4)) % P for q in range(n)] for k in range(4)])

    def coefficients(self, b):
        """B [4][n] -> a [4n]: the polynomial of degree < 4n whose values on the four even cosets those interpolants give"""
        n = b.shape[1]
        v = np.empty(4 * n, np.uint64)
        for kc in range(4):
            v[kc::4] = self.O.ntt(b[kc])
        return self.O.ntt(v, inverse=True)

    def odd_values(self, a):
        """a [4n] -> [4][n]: S on the odd cosets, y = w_8n^(2 kc + 1) w_n^j (point 8 j + 2 kc + 1 of <w_8n>)"""
        v = self.O.ntt(np.concatenate([a, np.zeros_like(a)]))
        return np.stack([v[2 * kc + 1::8] for kc in range(4)])

    def vector_of_values(self, values, k):
        """values on the coset w_8n^k <w_n> -> the vector the kernels write for it: the interpolant with the twist w_8n^(k q) taken out"""
        n = values.size
        return self.scale(self.O.ntt(values, inverse=True), pow(self.root(n.bit_length() + 2), -k, P))

    def values_of_vector(self, vec, k):
        """the transform the product runs on such a vector: prescale by w_8n^(k q), n-point transform"""
        n = vec.size
        return self.O.ntt(self.scale(vec, pow(self.root(n.bit_length() + 2), k, P)))

    # ---- even -> odd ---------------------------------------------------------------------------------------------------------------------
    def odd_vectors(self, a):
        """a [4n] -> [4][n], what coset_even_to_odd writes for the table"""
        vals = self.odd_values(a)
        return np.stack([self.vector_of_values(vals[kc], 2 * kc + 1) for kc in range(4)])

    def odd_vectors_closed(self, a):
        """out[kc][q] = sum_(i < 4) W8^(k' i) a_(q + n i), k' = 2 kc + 1"""
        a = self.ints(a)
        n = len(a) // 4
        w8 = pow(self.root(n.bit_length() + 2), n, P)
        return self.mont([[sum(pow(w8, (2 * kc + 1) * i, P) * a[q + n * i] for i in range(4)) % P for q in range(n)] for kc in range(4)])

    def window(self, b, kc0=0, nkc=4):
        """B with B_k := 0 for k outside [kc0, kc0 + nkc) (whatever words stand there)"""
        out = np.zeros_like(b)
        out[..., kc0:kc0 + nkc, :] = b[..., kc0:kc0 + nkc, :]
        return out

    def even_to_odd(self, d_in, kc0=0, nkc=4):
        """d_in [tables][4][n] -> [4 odd cosets][tables][n] for the window"""
        w = self.window(d_in, kc0, nkc)
        return np.stack([self.odd_vectors(self.coefficients(w[t])) for t in range(w.shape[0])], axis=1)

    # ---- merged ----------------------------------------------------------------------------------------------------------------------------
    def monomial(self, e, k, n, base=G):
        """(base z_j)^e on z_j = w_8n^k w_n^j, j < n"""
        key = ("x^e", e, k, n, base)
        if key not in self._tables:
            w8n, wn = self.root(n.bit_length() + 2), self.root(n.bit_length() - 1)
            shift = base * pow(w8n, k, P) % P
            self._tables[key] = self.mont([pow(shift * pow(wn, j, P) % P, e, P) for j in range(n)])
        return self._tables[key]

    def merged(self, d_in, families, raw_family=-1):
        """d_in [tables][4][n] of ONE set; families = [[(table, e), ...], ...] -> (out [4][families][n], raw [terms of raw_family][n] or
        None).  Family f = sum_t x^(e_t) S_t, x = g y: on odd coset k' its vector is the one of the values sum_t x_j^(e_t) S_t(x_j).  raw
        [t]: the interpolant of S_t over LDE coset 1, no twist taken out."""
        n = d_in.shape[2]
        used = sorted({t for fam in families for t, _ in fam})
        vals = {t: self.odd_values(self.coefficients(d_in[t])) for t in used}
        out = np.zeros((4, len(families), n), np.uint64)
        for kc in range(4):
            for f, fam in enumerate(families):
                acc = np.zeros(n, np.uint64)
                for t, e in fam:
                    acc = self.O.fp_add(acc, self.O.fp_mul(vals[t][kc], self.monomial(e, 2 * kc + 1, n)))
                out[kc, f] = self.vector_of_values(acc, 2 * kc + 1)
        raw = None
        if raw_family >= 0:
            raw = np.stack([self.O.ntt(vals[t][0], inverse=True) for t, _ in families[raw_family]])
        return out, raw

    def merge_constants(self, e, n, base=G, k0=1):
        """the host constants of one term, as integers: (c [4][2], r); c[i][0] = base^e W8^(k (d mod 8)), c[i][1] = c[i][0] W8^k with
        k = k0 + 2 i, d = e div n, r = e mod n"""
        w8 = pow(self.root(n.bit_length() + 2), n, P)
        d, r = divmod(e, n)
        c = []
        for i in range(4):
            k = k0 + 2 * i
            c0 = pow(base, e, P) * pow(w8, k * (d % 8), P) % P
            c.append([c0, c0 * pow(w8, k, P) % P])
        return c, r

    # ---- coset_combine ---------------------------------------------------------------------------------------------------------------------
    def combine_inputs(self, a, log_b):
        """coefficients a [B n] -> d_b [B][n]: the interpolants of the values over <w_N> on its cosets, value i = B j + k on coset k"""
        bb = 1 << log_b
        v = self.O.ntt(a)
        return np.stack([self.O.ntt(v[k::bb], inverse=True) for k in range(bb)])

    def combine(self, d_b):
        """d_b [B][n] -> d_h [B n]: d_h[i n + q] = a_(q + n i), the coefficients of the polynomial with those values"""
        bb, n = d_b.shape
        v = np.empty(bb * n, np.uint64)
        for k in range(bb):
            v[k::bb] = self.O.ntt(d_b[k])
        return self.O.ntt(v, inverse=True)

    # ---- the high part of the final addition --------------------------------------------------------------------------------------------------
    def halved_difference(self, t, q):
        inv2 = (P + 1) // 2
        return self.mont([(x - y) * inv2 % P for x, y in zip(self.ints(t), self.ints(q))]).reshape(np.shape(t))

    def final_hi(self, odd, direct, first, per_set, tables_per_set):
        """odd [sets tables_per_set][n] (the first coset block), direct [rows][n] -> hi [rows][n]"""
        rows = direct.shape[0]
        pick = [(r // per_set) * tables_per_set + first + r % per_set for r in range(rows)]
        return self.halved_difference(odd[pick], direct)

    def final_hi_merge(self, tco, qco, e, base, k0):
        """tco, qco [m][2][n] -> out [3][m][n]: with h0, h1 = (tco - qco) / 2 of slots 0, 1 as coefficient vectors in z, the vector on
        coset k = k0 + 2 i of the values h0(z) + (base z)^e h1(z), z = w_8n^k w_n^j"""
        m, _, n = tco.shape
        h = self.halved_difference(tco, qco)
        out = np.zeros((3, m, n), np.uint64)
        for i in range(3):
            k = k0 + 2 * i
            for c in range(m):
                v = self.O.fp_add(self.values_of_vector(h[c, 0], k), self.O.fp_mul(self.monomial(e, k, n, base), self.values_of_vector(h[c, 1], k)))
                out[i, c] = self.vector_of_values(v, k)
        return out

    # ---- the sharded path's data mover ----------------------------------------------------------------------------------------------------------
    def shard_combine(self, parts, nkc):
        """parts [4 / nkc][nkc + 4][n]: rank r's rows = its even cosets kc = r nkc + i, then its share of the four odd cosets -> out [8][n]:
        the even cosets from their owners, the odd ones summed over the ranks"""
        world, rows, n = parts.shape
        assert world == 4 // nkc and rows == nkc + 4
        out = np.zeros((8, n), np.uint64)
        for r in range(world):
            for i in range(nkc):
                out[2 * (r * nkc + i)] = parts[r, i]
        for kc in range(4):
            cols = [self.ints(parts[r, nkc + kc]) for r in range(world)]
            out[2 * kc + 1] = self.mont([sum(col[j] for col in cols) % P for j in range(n)])
        return out


def add_mod_p(ref, arrays):
    """element-wise sum of memory-form arrays (the Montgomery map is linear)"""
    acc = np.zeros_like(arrays[0])
    for a in arrays:
        acc = ref.O.fp_add(acc, a)
    return acc.reshape(arrays[0].shape)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def input_families(shape, rng):
    """memory-form words of that shape: random canonical, all p - 1, 0 and p - 1 alternating by index"""
    size = int(np.prod(shape))
    alt = np.zeros(size, np.uint64)
    alt[1::2] = P - 1
    return {"random": rng.integers(0, P, size=size, dtype=np.uint64).reshape(shape),
            "all p-1": np.full(shape, P - 1, np.uint64),
            "alternating": alt.reshape(shape)}


def impulse(ref, size, t):
    """the coefficient vector with a single 1 at t"""
    a = np.zeros(size, np.uint64)
    a[t] = ref.mont([1])[0]
    return a


def expected_buffer(words, values):
    """an output buffer of `words` words that started as FILL and received `values` at its start"""
    out = np.full(words, FILL_WORD, np.uint64)
    v = np.ascontiguousarray(values, np.uint64).reshape(-1)
    out[:v.size] = v
    return out


# ---- include/cstark_debug_coset.h ---------------------------------------------------------------------------------------------------------------
class MergeDescStruct(C.Structure):
    """struct cstark_debug_merge_desc"""
    _fields_ = [("families", C.c_uint32), ("tables_per_set", C.c_uint32), ("raw_family", C.c_int32), ("k0", C.c_uint32), ("base", C.c_uint64),
                ("terms", C.c_uint32 * MERGE_FAMILIES), ("table", (C.c_uint32 * MERGE_TERMS) * MERGE_FAMILIES),
                ("exponent", (C.c_uint64 * MERGE_TERMS) * MERGE_FAMILIES)]


class MergeTermStruct(C.Structure):
    """struct cstark_debug_merge_term"""
    _fields_ = [("c", (C.c_uint64 * 2) * 4), ("table", C.c_uint32), ("r", C.c_uint32)]


class CosetDev:
    """device buffers of a Backend's device as torch tensors, and the entry points of cstark_debug_coset.h on its context"""

    def __init__(self, backend):
        from certificate_stark_amd import _lib
        self.backend, self.lib = backend, _lib.load_debug()
        u32, u64, vp, sz = C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t
        self.lib.cstark_debug_even_to_odd.argtypes = [vp, vp, sz, vp, sz, u32, u32, u32, u32]
        self.lib.cstark_debug_even_to_odd_merged.argtypes = [vp, vp, sz, vp, sz, vp, sz, u32, u32, C.POINTER(MergeDescStruct), C.POINTER(MergeTermStruct)]
        self.lib.cstark_debug_coset_combine.argtypes = [vp, vp, vp, sz, u32, u32, u32]
        self.lib.cstark_debug_final_hi.argtypes = [vp, vp, sz, vp, sz, vp, sz, u32, u32, u32, u32, u32]
        self.lib.cstark_debug_final_hi_merge.argtypes = [vp, vp, vp, sz, vp, sz, u32, u32, u64, u64, u32, C.POINTER(MergeTermStruct)]
        self.lib.cstark_debug_shard_combine.argtypes = [vp, vp, sz, vp, sz, u32, u32]

    def u64(self, a):
        """a numpy array of words -> a flat device tensor"""
        return self.backend.from_numpy_u64(np.ascontiguousarray(a, np.uint64).reshape(-1))

    def filled(self, words):
        """an output buffer of `words` words, every byte FILL"""
        import torch
        return torch.full((words * 8,), FILL, dtype=torch.uint8, device=self.backend.device).view(torch.int64)

    @staticmethod
    def words_of(t):
        return t.cpu().numpy().view(np.uint64).reshape(-1)

    def even_to_odd(self, d_in, d_out, log_n, tables, kc0=0, nkc=4, in_words=None, out_words=None):
        return self.lib.cstark_debug_even_to_odd(self.backend.ctx, d_in.data_ptr(), d_in.numel() if in_words is None else in_words, d_out.data_ptr(),
                                                 d_out.numel() if out_words is None else out_words, log_n, tables, kc0, nkc)

    @staticmethod
    def merge_desc(families, tables_per_set, raw_family=-1, base_word=None, k0=1, terms=None):
        """families = [[(table, e), ...], ...]; base_word: memory form.  terms: term counts to state instead of the lists' lengths"""
        d = MergeDescStruct()
        d.families, d.tables_per_set, d.raw_family, d.k0, d.base = len(families), tables_per_set, raw_family, k0, int(base_word)
        for f, fam in enumerate(families[:MERGE_FAMILIES]):
            d.terms[f] = len(fam)
            for t, (table, e) in enumerate(fam[:MERGE_TERMS]):
                d.table[f][t], d.exponent[f][t] = table, e
        for f, count in (terms or {}).items():
            d.terms[f] = count
        return d

    def even_to_odd_merged(self, d_in, d_out, d_raw, log_n, sets, desc):
        """-> (status, terms [5][4] of (c [4][2], table, r) as built by the product)"""
        terms = (MergeTermStruct * (MERGE_FAMILIES * MERGE_TERMS))()
        rc = self.lib.cstark_debug_even_to_odd_merged(self.backend.ctx, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(),
                                                      d_raw.data_ptr() if d_raw is not None else None, d_raw.numel() if d_raw is not None else 0,
                                                      log_n, sets, C.byref(desc), terms)
        return rc, [[self._term(terms[f * MERGE_TERMS + t]) for t in range(MERGE_TERMS)] for f in range(MERGE_FAMILIES)]

    @staticmethod
    def _term(s):
        return [[int(s.c[i][0]), int(s.c[i][1])] for i in range(4)], int(s.table), int(s.r)

    def coset_combine(self, d_b, d_h, log_n, log_b, tables, words=None):
        return self.lib.cstark_debug_coset_combine(self.backend.ctx, d_b.data_ptr(), d_h.data_ptr(), min(d_b.numel(), d_h.numel()) if words is None else words,
                                                   log_n, log_b, tables)

    def final_hi(self, d_odd, d_direct, d_hi, log_n, rows, first, per_set, tables_per_set):
        return self.lib.cstark_debug_final_hi(self.backend.ctx, d_odd.data_ptr(), d_odd.numel(), d_direct.data_ptr(), d_direct.numel(), d_hi.data_ptr(),
                                              d_hi.numel(), log_n, rows, first, per_set, tables_per_set)

    def final_hi_merge(self, d_tco, d_qco, d_out, log_n, m, e, base_word, k0):
        term = MergeTermStruct()
        rc = self.lib.cstark_debug_final_hi_merge(self.backend.ctx, d_tco.data_ptr(), d_qco.data_ptr(), min(d_tco.numel(), d_qco.numel()), d_out.data_ptr(),
                                                  d_out.numel(), log_n, m, e, int(base_word), k0, C.byref(term))
        return rc, self._term(term)

    def shard_combine(self, d_parts, d_out, log_n, nkc):
        return self.lib.cstark_debug_shard_combine(self.backend.ctx, d_parts.data_ptr(), d_parts.numel(), d_out.data_ptr(), d_out.numel(), log_n, nkc)
