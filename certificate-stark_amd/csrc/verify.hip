// TransactionExample::verify (src/lib.rs:144-150) and the sub-AIR examples' verify (MerkleAir, RangeProofAir, RescueAir) for proofs in this
// library's own layout (include/cstark.h, "Proof layout"), many proofs per call, any mix of AIRs: what differs between the AIRs is the
// VAir record of each proof's descriptor, the constraint bodies (constraints.hip) and the cached periodic coefficients.  SchnorrAir
// (cstark_schnorr_verify) has an O(n) statement: it is staged behind the proof bytes, its channel seed is hashed on the host, and the 31
// statement-dependent values of the out-of-domain check -- the 19 public-input columns and the 12 sequence-assertion polynomials at z --
// are barycentric sums over the trace domain, formed in one pass by k_vfy_schnorr_public.  Pipeline of one chunk of proofs:
//   host    parse (structure only: every count against the stated options) and the per-proof constants of the domains; the raw
//           proof bytes and one descriptor per proof go to one pinned staging block -> ONE host-to-device copy
//   device  transcript replay, one workgroup per proof (Blake3 or Sha3 coin, vhash.cuh): coefficients, z, DEEP coefficients, layer
//           alphas, remainder commitment, proof of work, query positions and their folded positions and slots
//           per (AIR, extension degree m) present: (SchnorrAir: the statement's 31 values at z) -> out-of-domain frames (periodic columns at z^(n/cycle) from cached coefficients, the frame
//           sampled along t -> e(t) for m > 1) -> the AIR's constraints on every frame (constraints.hip, launch_eval_frames_air) -> merge
//           and compare with sum_i H_i z^i; DEEP + FRI, one lane per (proof, query)
//           all proofs: Merkle openings, one lane per opened row (leaf hash + path walk, Blake3 or Sha3) -- the trees of compact
//           proofs (proof_layout.h: one multiproof per tree) fold in one workgroup each instead (k_vfy_multi_open); remainder degree
//           (exact, one workgroup per component); reduction to one verdict per proof -> ONE device-to-host copy
// Every check writes one result slot with a plain store: the rank of its failure in the verdict order of cstark.h (or none); the
// reduction takes the smallest.  The number of launches per chunk does not depend on the number of proofs.
#include <hip/hip_runtime.h>
#include <string.h>
#include <assert.h>
#include <algorithm>
#include <array>
#include <type_traits>
#include <chrono>
#include <vector>
#include "../../include/cstark.h"
#include "ctx.h"
#include "constraints.h"
#include "air_tx_host.h"
#include "coin.h"
#include "proof_layout.h"
#include "transcript.h"
#include "blake3_compress.cuh"
#include "ext.cuh"
#include "keccak.cuh"
#include "vhash.cuh"

namespace cs {

// failure ranks: smaller = earlier in the verdict order of cstark.h
enum : uint32_t {
    RK_MALFORMED = 0, RK_OOD = 1, RK_REMAINDER_COMMITMENT = 2, RK_POW = 3,
    RK_OPENING0 = 4,     // + 2 q (+ 1 for the composition opening)
    RK_LAYER0 = 1000,    // + 3 l + (0 count, 1 opening, 2 folding)
    RK_REMAINDER_FOLDING = 2000, RK_REMAINDER_DEGREE = 2001,
    RK_NONE = 0xffffffffu
};

// ---- what the device reads --------------------------------------------------------------------------------------------------------
// What the pipeline knows of an AIR (host: air_desc; every proof's descriptor carries a copy): trace width | composition columns =
// constraint-evaluation blowup | transition constraints | single-row assertions | public words in the channel seed | periodic columns
// and the binary logarithm of their cycle | the first asserted register.  Assertion a < na / 2 is on register areg + a at row 0,
// assertion na / 2 + a on the same register at row n - 1; their values are the descriptor's K_PUB words, in that order.
// naux: frame entries beyond the periodic ones that depend on the statement (SchnorrAir's 19 public-input columns at z).
struct VAir { uint32_t air, w, ce, nc, na, npub, nper, log_cycle, areg, naux; };
constexpr uint32_t VMAX_NC = 115, VMAX_NPER = 56, VMAX_GROUPS = 8;
// SchnorrAir's assertions (air_groups.h, air_shape(2)) as the merge reads them: register, divisor group (0: step 0, 1: step 511 of every
// 512-row block) and value (0, 1: the constants zero and one; 2 + q: sequence value q of the statement)
constexpr uint32_t VMAX_NA = 61, SCH_PUBLIC = 31, SCH_AUX = 19, SCH_TILE = 4; // SCH_TILE signatures (waves) per workgroup of k_vfy_schnorr_public
struct VAsserts { uint8_t n, reg[VMAX_NA], div[VMAX_NA], val[VMAX_NA]; };
// the degree-adjustment group of every constraint of one AIR (k_vfy_ood_check's argument; the exponents are K_ADJ of the proof)
struct VGroups { uint8_t n, g[VMAX_NC]; };

// Offsets (in words) of the replayed transcript block of a proof (device memory, written by k_vfy_transcript): z | t_alpha, t_beta [nc] | b_alpha, b_beta [na] | DEEP alpha, beta [w]
// | delta [ce] | deg_a | deg_b | layer alphas [L] (all m words each) | constants | positions [nq] | slots [L][nq] | folded positions [L][nq]
struct TOff { uint32_t z, ta, tb, ba, bb, da, db, dd, dga, dgb, alpha, k, pos, slot, lpos, st, words; };
enum { K_WN, K_WNN, K_WLAST, K_G, K_ADJ /* [VMAX_GROUPS] */, K_BADJ = K_ADJ + 8, K_INVF, K_ZETA_INV, K_WRINV, K_PUB /* [14] */, K_WL = K_PUB + 14 /* [L] */, K_WORDS = K_WL + VMAX_LAYERS };
__host__ __device__ inline TOff toff(const VAir &a, uint32_t m, uint32_t L, uint32_t nq) {
    TOff t;
    uint32_t o = 0;
    t.z = o; o += m;
    t.ta = o; o += a.nc * m; t.tb = o; o += a.nc * m; t.ba = o; o += a.na * m; t.bb = o; o += a.na * m;
    t.da = o; o += a.w * m; t.db = o; o += a.w * m; t.dd = o; o += a.ce * m; t.dga = o; o += m; t.dgb = o; o += m;
    t.alpha = o; o += L * m;
    t.k = o; o += K_WORDS;
    t.pos = o; o += nq; t.slot = o; o += L * nq; t.lpos = o; o += L * nq;
    t.st = o; o += 2; // layers whose count matched the derived positions | the first failure found by the replay (rank)
    t.words = o;
    return t;
}

struct VDesc {
    uint64_t base;   // byte offset of the proof in the chunk's block (8-aligned)
    uint64_t tb;     // word offset of its transcript block in the device region
    uint64_t k[K_WORDS];  // constants of its domains (host; copied to the transcript block)
    uint64_t pub[14];     // the public words of the channel seed, memory form (a.npub of them)
    uint64_t pcoef;       // word offset of the AIR's periodic coefficients [a.nper][2^a.log_cycle] in the cache
    uint64_t stmt;        // SchnorrAir: byte offset of the statement in the chunk's block, messages [n_sig][28] | R.x [n_sig][6] | s [n_sig][32]
    uint64_t sp;          // ... word offset of its public values in the device region: partials [tiles][31][m], then the values [31][m]
    uint32_t seed[8];     // ... the channel seed's digest (host: transcript.h, channel_seed)
    uint32_t n_sig;
    VAir a;
    uint32_t ood, trows, tpaths, crows, cpaths, rem;                 // byte offsets inside the proof
    uint32_t lrows[VMAX_LAYERS];
    uint32_t log_n, log_N, nq, log_f, n_layers, m, R, log_b, hash, grinding, log_rem, npos[VMAX_LAYERS];
    uint32_t slot0;     // result slots: [0] out-of-domain, then openings, then nq queries, then m remainder components
    uint32_t n_open;    // opening slots: one per opened row, or (compact proof) one per tree
};
__device__ __forceinline__ TOff toff(const VDesc &d) { return toff(d.a, d.m, d.n_layers, d.nq); }
struct VOpen {
    uint32_t proof, row, path, root; // row / path / root: byte offsets inside the proof
    uint32_t words, depth, layer, t, rank, slot, hash; // layer = VNO_LAYER: trace / composition row of query t; else row t of that layer
};
constexpr uint32_t VNO_LAYER = 0xffffffffu;
// one tree of a compact proof: `count` opened rows of `words` words from byte offset `rows` on, `n_nodes` multiproof nodes from `nodes` on
struct VMulti {
    uint32_t proof, rows, nodes, n_nodes, root; // byte offsets inside the proof (and the stated node count)
    uint32_t words, depth, layer, count, rank, slot, hash; // layer = VNO_LAYER: the trace / composition tree; else that layer's
};

// ---- device helpers ---------------------------------------------------------------------------------------------------------------
// proof bytes are 4-aligned only (each layer's count word shifts what follows by 4)
__device__ __forceinline__ uint64_t ld64(const uint8_t *p) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    return (uint64_t)q[0] | ((uint64_t)q[1] << 32);
}
template <int M> __device__ __forceinline__ Ext<M> ld_ext(const uint8_t *p) { Ext<M> r; for (int i = 0; i < M; i++) r.c[i] = ld64(p + 8 * i); return r; }
template <int M> __device__ __forceinline__ Ext<M> x_base(fp v) { Ext<M> r = x_zero<M>(); r.c[0] = v; return r; }
template <int M> __device__ __forceinline__ bool x_eq(const Ext<M> &a, const Ext<M> &b) {
    bool e = true;
    for (int i = 0; i < M; i++) e &= a.c[i] == b.c[i];
    return e;
}

// Blake3 of `words` 64-bit words (one chunk: at most 128 words); canonical &= every word < p
__device__ void b3_words(const uint8_t *p, uint32_t words, uint32_t (&cv)[8], bool &canonical) {
    cv[0] = IV0; cv[1] = IV1; cv[2] = IV2; cv[3] = IV3; cv[4] = IV4; cv[5] = IV5; cv[6] = IV6; cv[7] = IV7;
    const uint32_t nb = (words + 7) / 8;
    for (uint32_t bk = 0; bk < nb; bk++) {
        uint32_t m[16];
        const uint32_t cnt = words - 8 * bk < 8 ? words - 8 * bk : 8;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint64_t v = 0;
            if ((uint32_t)i < cnt) {
                v = ld64(p + 8 * (8 * bk + i));
                canonical &= v < FP_P;
#if !CSTARK_CONV_HASHED_ELEMENT_BYTES_MONTGOMERY
                v = fp_to_u64(v);
#endif
            }
            m[2 * i] = (uint32_t)v;
            m[2 * i + 1] = (uint32_t)(v >> 32);
        }
        compress(cv, m, cnt * 8, (bk == 0 ? CHUNK_START : 0u) | (bk + 1 == nb ? (CHUNK_END | ROOT) : 0u));
    }
}
// SHA3-256 of `words` 64-bit words (the state stays in registers: every lane index below is a compile-time constant)
__device__ void sha3_words(const uint8_t *p, uint32_t words, uint64_t (&h)[4], bool &canonical) {
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
    for (uint32_t w0 = 0;; w0 += 17) {
        const uint32_t cnt = words - w0 < 17 ? words - w0 : 17; // a full block is followed by at least the padding block
#pragma unroll
        for (uint32_t i = 0; i < 17; i++)
            if (i < cnt) {
                uint64_t v = ld64(p + 8 * (w0 + i));
                canonical &= v < FP_P;
#if !CSTARK_CONV_HASHED_ELEMENT_BYTES_MONTGOMERY
                v = fp_to_u64(v);
#endif
                s[i] ^= v;
            }
        if (cnt < 17) {
#pragma unroll
            for (uint32_t i = 0; i < 17; i++) if (i == cnt) s[i] ^= 0x06;
            s[16] ^= 0x80ull << 56;
            keccak::permute(s);
            break;
        }
        keccak::permute(s);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) h[i] = s[i];
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
// One lane per opened row: leaf hash, path walk, comparison with the root.  The list is sorted by (hash, leaf words, path length).
// Leaf positions come from the replayed transcript; rows of layers from the first one whose count differs are checked for canonical
// words only.
__global__ __launch_bounds__(128) void k_vfy_openings(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const VOpen *__restrict__ opens,
                                                      uint32_t n_open, const uint64_t *__restrict__ tbase, uint32_t *__restrict__ slots) {
    const uint32_t t = blockIdx.x * 128 + threadIdx.x;
    if (t >= n_open) return;
    const VOpen o = opens[t];
    const VDesc &d = desc[o.proof];
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    bool canonical = true, match = true;
    uint32_t idx = 0, rank = o.rank;
    if (o.layer == VNO_LAYER) idx = (uint32_t)tb[to.pos + o.t];
    else if (o.layer < (uint32_t)tb[to.st]) idx = (uint32_t)tb[to.lpos + o.layer * d.nq + o.t];
    else rank = RK_NONE;
    if (o.hash == 0) {
        uint32_t cv[8];
        b3_words(pb + o.row, o.words, cv, canonical);
        for (uint32_t lvl = 0; lvl < o.depth; lvl++) {
            const uint32_t *sib = reinterpret_cast<const uint32_t *>(pb + o.path + 32 * lvl);
            uint32_t m[16];
            const bool right = idx & 1;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t sv = sib[i];
                m[i] = right ? sv : cv[i];
                m[8 + i] = right ? cv[i] : sv;
            }
            cv[0] = IV0; cv[1] = IV1; cv[2] = IV2; cv[3] = IV3; cv[4] = IV4; cv[5] = IV5; cv[6] = IV6; cv[7] = IV7;
            compress(cv, m, 64, CHUNK_START | CHUNK_END | ROOT);
            idx >>= 1;
        }
        const uint32_t *root = reinterpret_cast<const uint32_t *>(pb + o.root);
        for (int i = 0; i < 8; i++) match &= cv[i] == root[i];
    } else {
        uint64_t h[4];
        sha3_words(pb + o.row, o.words, h, canonical);
        for (uint32_t lvl = 0; lvl < o.depth; lvl++) {
            const uint8_t *sib = pb + o.path + 32 * lvl;
            uint64_t s[25];
#pragma unroll
            for (int i = 0; i < 25; i++) s[i] = 0;
            const bool right = idx & 1;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint64_t sv = ld64(sib + 8 * i);
                s[i] = right ? sv : h[i];
                s[4 + i] = right ? h[i] : sv;
            }
            s[8] ^= 0x06;
            s[16] ^= 0x80ull << 56;
            keccak::permute(s);
            for (int i = 0; i < 4; i++) h[i] = s[i];
            idx >>= 1;
        }
        const uint8_t *root = pb + o.root;
        for (int i = 0; i < 4; i++) match &= h[i] == ld64(root + 8 * i);
    }
    slots[o.slot] = !canonical ? (uint32_t)RK_MALFORMED : match ? (uint32_t)RK_NONE : rank;
}

// ---- the multiproof of one tree of a compact proof ----------------------------------------------------------------------------------
// Digests travel as eight 32-bit words under either hash.  The parent of two digests, as k_vfy_openings forms it.
template <int HASH> __device__ __forceinline__ void multi_parent(const uint32_t (&l)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
    if constexpr (HASH == 0) {
        uint32_t m[16];
#pragma unroll
        for (int i = 0; i < 8; i++) { m[i] = l[i]; m[8 + i] = r[i]; }
        out[0] = IV0; out[1] = IV1; out[2] = IV2; out[3] = IV3; out[4] = IV4; out[5] = IV5; out[6] = IV6; out[7] = IV7;
        compress(out, m, 64, CHUNK_START | CHUNK_END | ROOT);
    } else {
        uint64_t s[25]; // in registers: every lane index is a compile-time constant
#pragma unroll
        for (int i = 0; i < 25; i++) s[i] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s[i] = (uint64_t)l[2 * i] | ((uint64_t)l[2 * i + 1] << 32);
            s[4 + i] = (uint64_t)r[2 * i] | ((uint64_t)r[2 * i + 1] << 32);
        }
        s[8] ^= 0x06;
        s[16] ^= 0x80ull << 56;
        keccak::permute(s);
#pragma unroll
        for (int i = 0; i < 4; i++) { out[2 * i] = (uint32_t)s[i]; out[2 * i + 1] = (uint32_t)(s[i] >> 32); }
    }
}
// Order-preserving positions of the threads that flag a (pa) and b (pb) among the 128 of the workgroup, and the two totals: a ballot per
// wave, the other wave's counts through LDS (compact_position of channel.hip, two flags at once).  Called by all threads; the caller
// synchronises before the next call (it does anyway, after writing what the positions index).
__device__ __forceinline__ void multi_scan(uint32_t (&cnt)[2][2], bool a, bool b, uint32_t &pa, uint32_t &pb, uint32_t &ta, uint32_t &tb) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t va = __ballot(a), vb = __ballot(b), below = (1ull << lane) - 1;
    if (lane == 0) { cnt[wave][0] = (uint32_t)__popcll(va); cnt[wave][1] = (uint32_t)__popcll(vb); }
    __syncthreads();
    pa = (wave ? cnt[0][0] : 0u) + (uint32_t)__popcll(va & below);
    pb = (wave ? cnt[0][1] : 0u) + (uint32_t)__popcll(vb & below);
    ta = cnt[0][0] + cnt[1][0];
    tb = cnt[0][1] + cnt[1][1];
}
// One workgroup of 128 threads per tree (HASH: 0 Blake3, 1 Sha3; the list holds the trees of one hash).  Positions come from the replayed
// transcript, as in k_vfy_openings; a layer from the first one whose count differs has its rows checked for canonical words only.
//   1 leaves    thread t < count hashes row t (proof order)
//   2 sort      the rank of every position among the count <= 128 (O(n^2) over LDS); equal positions must carry equal digests and
//               collapse to one entry
//   3 fold      for l = depth .. 1: entry i of K_l (ascending) is the left half of a pair inside K_l, its right half, or single; a single
//               takes the next proof node -- its index is the number of singles before it (multi_scan) behind the nodes of the levels
//               below; every entry but a right half hashes one parent into the other buffer, at its position among those
//   4 verdict   accepted iff exactly n_nodes nodes were consumed and the last digest is the committed root
// Everything a thread indexes is bounded by count <= 128 (parse_layout: num_queries, n_positions) and, for the proof nodes, by the
// stated n_nodes, which parse_layout has placed inside the proof; no flags between workgroups, no atomics.
template <int HASH>
__global__ __launch_bounds__(128) void k_vfy_multi_open(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const VMulti *__restrict__ trees,
                                                        const uint64_t *__restrict__ tbase, uint32_t *__restrict__ slots) {
    __shared__ uint32_t dig[2][128][8];
    __shared__ uint32_t key[2][128];
    __shared__ uint32_t cnt[2][2];
    const VMulti o = trees[blockIdx.x];
    const VDesc &d = desc[o.proof];
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const uint32_t tid = threadIdx.x;
    const bool placed = o.layer == VNO_LAYER || o.layer < (uint32_t)tb[to.st]; // uniform: the tree's positions are known
    bool canonical = true, bad = false;
    uint32_t cv[8] = {}, pos = 0xffffffffu;
    if (tid < o.count) {
        const uint8_t *row = pb + o.rows + 8 * (size_t)tid * o.words;
        if constexpr (HASH == 0) b3_words(row, o.words, cv, canonical);
        else {
            uint64_t h[4];
            sha3_words(row, o.words, h, canonical);
#pragma unroll
            for (int i = 0; i < 4; i++) { cv[2 * i] = (uint32_t)h[i]; cv[2 * i + 1] = (uint32_t)(h[i] >> 32); }
        }
        if (placed) pos = o.layer == VNO_LAYER ? (uint32_t)tb[to.pos + tid] : (uint32_t)tb[to.lpos + o.layer * d.nq + tid];
    }
    key[0][tid] = pos;
    const int malformed = __syncthreads_or(!canonical);
    if (malformed || !placed) {
        if (tid == 0) slots[o.slot] = malformed ? (uint32_t)RK_MALFORMED : (uint32_t)RK_NONE;
        return;
    }
    // ---- sort into buffer 1, collapse into buffer 0
    if (tid < o.count) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < o.count; j++) {
            const uint32_t kj = key[0][j];
            r += (kj < pos || (kj == pos && j < tid)) ? 1u : 0u;
        }
        key[1][r] = pos;
#pragma unroll
        for (int i = 0; i < 8; i++) dig[1][r][i] = cv[i];
    }
    __syncthreads();
    uint32_t n, used = 0;
    {
        bool first = false;
        if (tid < o.count) {
            pos = key[1][tid];
            first = tid == 0 || key[1][tid - 1] != pos;
#pragma unroll
            for (int i = 0; i < 8; i++) { cv[i] = dig[1][tid][i]; if (!first) bad |= cv[i] != dig[1][tid - 1][i]; }
        }
        uint32_t at, unused0, unused1;
        multi_scan(cnt, first, false, at, unused0, n, unused1);
        if (first) {
            key[0][at] = pos;
#pragma unroll
            for (int i = 0; i < 8; i++) dig[0][at][i] = cv[i];
        }
        __syncthreads();
    }
    // ---- fold
    uint32_t cur = 0;
    for (uint32_t l = o.depth; l >= 1; l--) {
        const bool in = tid < n;
        const uint32_t x = in ? key[cur][tid] : 0u;
        const bool right_half = in && (x & 1) && tid > 0 && key[cur][tid - 1] == x - 1;
        const bool left_half = in && !(x & 1) && tid + 1 < n && key[cur][tid + 1] == x + 1;
        const bool parent = in && !right_half, single = parent && !left_half;
        uint32_t at, node, n_next, n_single;
        multi_scan(cnt, parent, single, at, node, n_next, n_single);
        if (parent) {
            uint32_t own[8], sib[8], out[8];
#pragma unroll
            for (int i = 0; i < 8; i++) own[i] = dig[cur][tid][i];
            if (left_half) {
#pragma unroll
                for (int i = 0; i < 8; i++) sib[i] = dig[cur][tid + 1][i];
            } else if (used + node < o.n_nodes) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(pb + o.nodes + 32 * (size_t)(used + node));
#pragma unroll
                for (int i = 0; i < 8; i++) sib[i] = src[i];
            } else { // the proof states fewer nodes than the positions ask for
                bad = true;
#pragma unroll
                for (int i = 0; i < 8; i++) sib[i] = 0;
            }
            if (x & 1) multi_parent<HASH>(sib, own, out);
            else multi_parent<HASH>(own, sib, out);
            key[cur ^ 1][at] = x >> 1;
#pragma unroll
            for (int i = 0; i < 8; i++) dig[cur ^ 1][at][i] = out[i];
        }
        __syncthreads();
        n = n_next; used += n_single; cur ^= 1;
    }
    // ---- verdict
    if (tid == 0) {
        const uint32_t *root = reinterpret_cast<const uint32_t *>(pb + o.root);
        bad |= n != 1 || used != o.n_nodes;
        for (int i = 0; i < 8; i++) bad |= dig[cur][0][i] != root[i];
    }
    const int refused = __syncthreads_or(bad);
    if (tid == 0) slots[o.slot] = refused ? o.rank : (uint32_t)RK_NONE;
}

// ---- conversion between the proof forms (cstark_*_convert) -------------------------------------------------------------------------
// The leaf digest of an opened row as eight words, the leaf step of k_vfy_multi_open.
template <int HASH> __device__ __forceinline__ void multi_leaf(const uint8_t *row, uint32_t words, uint32_t (&cv)[8], bool &canonical) {
    if constexpr (HASH == 0) b3_words(row, words, cv, canonical);
    else {
        uint64_t h[4];
        sha3_words(row, words, h, canonical);
#pragma unroll
        for (int i = 0; i < 4; i++) { cv[2 * i] = (uint32_t)h[i]; cv[2 * i + 1] = (uint32_t)(h[i] >> 32); }
    }
}
// Compact -> plain: k_vfy_multi_open for a tree whose proof is being expanded, launched instead of it: the same leaves, sort, collapse,
// fold and result slot, and beside them the tree's paths [count][depth][32] at byte out_at[blockIdx.x] of the output block `outb` (the
// host sized that region from the parsed layout; out_at is a multiple of 32).  The paths fall out of the fold: at level l every entry of the ascending
// list knows its sibling digest -- the neighbouring entry of a pair, or the proof node a single consumes -- and where its parent lands
// in the next list (its own `at`; a right half: its left neighbour's, at - 1).  Both go to LDS (sib, nxt); the thread of opened row q
// holds the index of the entry its position is below, stores that entry's sibling as entry depth - l of path q and follows nxt.  The
// sorted list is treated alike: nxt of sorted place r is the entry it collapsed to, so equal positions get equal paths.  A refused tree
// writes nothing or digests it has in hand, inside its own region; a node index at or past n_nodes is never read.
template <int HASH>
__global__ __launch_bounds__(128) void k_vfy_multi_expand(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const VMulti *__restrict__ trees,
                                                          const uint64_t *__restrict__ tbase, uint32_t *__restrict__ slots,
                                                          const uint64_t *__restrict__ out_at, uint8_t *__restrict__ outb) {
    __shared__ uint32_t dig[2][128][8];
    __shared__ uint32_t key[2][128];
    __shared__ uint32_t sib[128][8];
    __shared__ uint32_t nxt[128];
    __shared__ uint32_t cnt[2][2];
    const VMulti o = trees[blockIdx.x];
    const VDesc &d = desc[o.proof];
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const uint32_t tid = threadIdx.x;
    const bool placed = o.layer == VNO_LAYER || o.layer < (uint32_t)tb[to.st]; // uniform: the tree's positions are known
    bool canonical = true, bad = false;
    uint32_t cv[8] = {}, pos = 0xffffffffu;
    if (tid < o.count) {
        multi_leaf<HASH>(pb + o.rows + 8 * (size_t)tid * o.words, o.words, cv, canonical);
        if (placed) pos = o.layer == VNO_LAYER ? (uint32_t)tb[to.pos + tid] : (uint32_t)tb[to.lpos + o.layer * d.nq + tid];
    }
    key[0][tid] = pos;
    const int malformed = __syncthreads_or(!canonical);
    if (malformed || !placed) {
        if (tid == 0) slots[o.slot] = malformed ? (uint32_t)RK_MALFORMED : (uint32_t)RK_NONE;
        return;
    }
    // ---- sort into buffer 1, collapse into buffer 0
    uint32_t entry = 0; // row tid's place in the list at hand: sorted place, then the entry above it level by level
    if (tid < o.count) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < o.count; j++) {
            const uint32_t kj = key[0][j];
            r += (kj < pos || (kj == pos && j < tid)) ? 1u : 0u;
        }
        key[1][r] = pos;
#pragma unroll
        for (int i = 0; i < 8; i++) dig[1][r][i] = cv[i];
        entry = r;
    }
    __syncthreads();
    uint32_t n, used = 0;
    {
        bool first = false;
        if (tid < o.count) {
            pos = key[1][tid];
            first = tid == 0 || key[1][tid - 1] != pos;
#pragma unroll
            for (int i = 0; i < 8; i++) { cv[i] = dig[1][tid][i]; if (!first) bad |= cv[i] != dig[1][tid - 1][i]; }
        }
        uint32_t at, unused0, unused1;
        multi_scan(cnt, first, false, at, unused0, n, unused1);
        if (first) {
            key[0][at] = pos;
#pragma unroll
            for (int i = 0; i < 8; i++) dig[0][at][i] = cv[i];
        }
        if (tid < o.count) nxt[tid] = first ? at : at - 1; // not first: tid > 0 and a first lies before it, so at >= 1
        __syncthreads();
        if (tid < o.count) entry = nxt[entry];
    }
    // ---- fold
    uint8_t *paths = outb + out_at[blockIdx.x] + 32 * (size_t)tid * o.depth; // row tid's path (tid < count)
    uint32_t cur = 0;
    for (uint32_t l = o.depth; l >= 1; l--) {
        const bool in = tid < n;
        const uint32_t x = in ? key[cur][tid] : 0u;
        const bool right_half = in && (x & 1) && tid > 0 && key[cur][tid - 1] == x - 1;
        const bool left_half = in && !(x & 1) && tid + 1 < n && key[cur][tid + 1] == x + 1;
        const bool parent = in && !right_half, single = parent && !left_half;
        uint32_t at, node, n_next, n_single;
        multi_scan(cnt, parent, single, at, node, n_next, n_single); // its barrier: every row has read sib and nxt of the level below
        if (in) {
            uint32_t own[8], sb[8];
            const uint32_t other = right_half ? tid - 1 : tid + 1;
#pragma unroll
            for (int i = 0; i < 8; i++) own[i] = dig[cur][tid][i];
            if (left_half || right_half) {
#pragma unroll
                for (int i = 0; i < 8; i++) sb[i] = dig[cur][other][i];
            } else if (used + node < o.n_nodes) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(pb + o.nodes + 32 * (size_t)(used + node));
#pragma unroll
                for (int i = 0; i < 8; i++) sb[i] = src[i];
            } else { // the proof states fewer nodes than the positions ask for
                bad = true;
#pragma unroll
                for (int i = 0; i < 8; i++) sb[i] = 0;
            }
#pragma unroll
            for (int i = 0; i < 8; i++) sib[tid][i] = sb[i];
            nxt[tid] = right_half ? at - 1 : at; // a right half: its left neighbour is a parent before it, so at >= 1
            if (parent) {
                uint32_t out[8];
                if (x & 1) multi_parent<HASH>(sb, own, out);
                else multi_parent<HASH>(own, sb, out);
                key[cur ^ 1][at] = x >> 1;
#pragma unroll
                for (int i = 0; i < 8; i++) dig[cur ^ 1][at][i] = out[i];
            }
        }
        __syncthreads();
        if (tid < o.count) { // entry < n: it came from nxt of the level below, which is below n_next there
            uint4 *dst = reinterpret_cast<uint4 *>(paths + 32 * (size_t)(o.depth - l));
            dst[0] = make_uint4(sib[entry][0], sib[entry][1], sib[entry][2], sib[entry][3]);
            dst[1] = make_uint4(sib[entry][4], sib[entry][5], sib[entry][6], sib[entry][7]);
            entry = nxt[entry];
        }
        n = n_next; used += n_single; cur ^= 1;
    }
    // ---- verdict
    if (tid == 0) {
        const uint32_t *root = reinterpret_cast<const uint32_t *>(pb + o.root);
        bad |= n != 1 || used != o.n_nodes;
        for (int i = 0; i < 8; i++) bad |= dig[cur][0][i] != root[i];
    }
    const int refused = __syncthreads_or(bad);
    if (tid == 0) slots[o.slot] = refused ? o.rank : (uint32_t)RK_NONE;
}

// Plain -> compact: one tree of a plain proof that is being compacted (its verdict stays k_vfy_openings').  paths: byte offset of the
// tree's paths [count][depth][32] inside the proof; the selected nodes go to byte `out` of the output block (room for count * depth of
// them) and their number to counts[index].
struct VSelect { uint32_t proof, paths, depth, layer, count, index; uint64_t out; };
// One workgroup of 128 threads per tree, no hashing: select_multiproof (proof_layout.h) on the device.  The positions are ranked and
// collapsed in LDS as in k_vfy_multi_open, every entry carrying one row below it (of equal positions the first in proof order, of a
// pair the left half's, as the host's `below`); the levels are walked on the keys alone, and a single entry x at level l copies entry
// depth - l of its row's path -- node (l, x ^ 1) -- to node slot used + node.  A layer from the first one whose count differs from the
// derived positions has none (the proof's verdict is LAYER_COUNT and it is not converted): its count stays 0.
__global__ __launch_bounds__(128) void k_vfy_multi_select(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const VSelect *__restrict__ trees,
                                                          const uint64_t *__restrict__ tbase, uint32_t *__restrict__ counts, uint8_t *__restrict__ outb) {
    __shared__ uint32_t key[2][128];
    __shared__ uint32_t row[2][128];
    __shared__ uint32_t cnt[2][2];
    const VSelect o = trees[blockIdx.x];
    const VDesc &d = desc[o.proof];
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const uint32_t tid = threadIdx.x;
    if (o.layer != VNO_LAYER && o.layer >= (uint32_t)tb[to.st]) { // uniform
        if (tid == 0) counts[o.index] = 0;
        return;
    }
    uint32_t pos = 0xffffffffu;
    if (tid < o.count) pos = o.layer == VNO_LAYER ? (uint32_t)tb[to.pos + tid] : (uint32_t)tb[to.lpos + o.layer * d.nq + tid];
    key[0][tid] = pos;
    __syncthreads();
    if (tid < o.count) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < o.count; j++) {
            const uint32_t kj = key[0][j];
            r += (kj < pos || (kj == pos && j < tid)) ? 1u : 0u;
        }
        key[1][r] = pos;
        row[1][r] = tid;
    }
    __syncthreads();
    uint32_t n, used = 0;
    {
        bool first = false;
        uint32_t q = 0;
        if (tid < o.count) {
            pos = key[1][tid];
            q = row[1][tid];
            first = tid == 0 || key[1][tid - 1] != pos;
        }
        uint32_t at, unused0, unused1;
        multi_scan(cnt, first, false, at, unused0, n, unused1);
        if (first) { key[0][at] = pos; row[0][at] = q; }
        __syncthreads();
    }
    const uint32_t room = o.count * o.depth; // node slots of the tree's region
    uint32_t cur = 0;
    for (uint32_t l = o.depth; l >= 1; l--) {
        const bool in = tid < n;
        const uint32_t x = in ? key[cur][tid] : 0u, q = in ? row[cur][tid] : 0u;
        const bool right_half = in && (x & 1) && tid > 0 && key[cur][tid - 1] == x - 1;
        const bool left_half = in && !(x & 1) && tid + 1 < n && key[cur][tid + 1] == x + 1;
        const bool parent = in && !right_half, single = parent && !left_half;
        uint32_t at, node, n_next, n_single;
        multi_scan(cnt, parent, single, at, node, n_next, n_single);
        if (single && used + node < room) { // always: a multiproof never holds more nodes than the paths it is selected from
            const uint32_t *src = reinterpret_cast<const uint32_t *>(pb + o.paths + 32 * ((size_t)q * o.depth + (o.depth - l)));
            uint4 *dst = reinterpret_cast<uint4 *>(outb + o.out + 32 * (size_t)(used + node));
            dst[0] = make_uint4(src[0], src[1], src[2], src[3]);
            dst[1] = make_uint4(src[4], src[5], src[6], src[7]);
        }
        if (parent) { key[cur ^ 1][at] = x >> 1; row[cur ^ 1][at] = q; }
        __syncthreads();
        n = n_next; used += n_single; cur ^= 1;
    }
    if (tid == 0) counts[o.index] = used < room ? used : room;
}

template <int R, class F> __device__ __forceinline__ void static_down(F &&f) {
    f(std::integral_constant<int, R>{});
    if constexpr (R > 0) static_down<R - 1>(f);
}
__host__ __device__ inline uint32_t schnorr_tiles(uint32_t n_sig) { return (n_sig + SCH_TILE - 1) / SCH_TILE; }

// SchnorrAir's statement at z.  With w = w_n, n = 512 T, and term_i = w^i / (z - w^i), every column that is non-zero on rows R only has
// the value (z^n - 1) / n * sum_{i in R} v_i term_i at z, and a sequence polynomial (degree < T, values on the coset w^first <w^512>)
// the value (z^T w^(-first T) - 1) / T * sum_t v_t term_{512 t + first}.  This kernel forms the sums: grid (tiles, proofs of the group),
// one wave per signature (512 rows), lane l rows 8 l .. 8 l + 7: one inversion per lane (prefix products), the block sum S_t through
// shared memory, the six single terms (rows 0, 7, 15, 23, 31, 511) beside it, then lanes 0..30 form the signature's 31 contributions:
//   0..11   public key word j: msg[t][j] S_t                  12..18  hash input j: sum_{i<4} msg[t][j + 7 i] term_{512 t + 8 i + 7}
//   19..24  R.x word k at step 0: rx[t][k] term_{512 t}       25..30  at step 511: rx[t][k] term_{512 t + 511}
// The workgroup's SCH_TILE signatures are added in shared memory; its partial [31][M] goes out with plain stores (no atomics on field
// elements) and k_vfy_schnorr_public_sum adds the tiles and applies the two factors.  Every bound is the descriptor's n_sig, which the
// host took from the validated header.
template <int M>
__global__ __launch_bounds__(64 * SCH_TILE) void k_vfy_schnorr_public(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc,
                                                                      const uint32_t *__restrict__ gp, const uint64_t *__restrict__ tbase,
                                                                      uint64_t *__restrict__ spub) {
    __shared__ Ext<M> red[SCH_TILE][64];
    __shared__ Ext<M> spec[SCH_TILE][7];        // term of row 0, 7, 15, 23, 31, 511 of the block | S_t
    __shared__ Ext<M> contrib[SCH_TILE][32];
    const VDesc &d = desc[gp[blockIdx.y]];
    const uint32_t T = d.n_sig;
    if (blockIdx.x >= schnorr_tiles(T)) return; // the grid is sized for the group's largest statement (uniform per workgroup)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * SCH_TILE + wave;
    const bool live = t < T;
    const Ext<M> z = x_load<M>(tbase + d.tb + toff(d).z);
    const fp wn = d.k[K_WN];
    Ext<M> sum = x_zero<M>();
    if (live) {
        fp w[8];
        Ext<M> dif[8], pre[8];
        // w_n^(512 t + 8 lane), row < 2^21: every lane takes the same 21 steps (a loop that ends with the lane's exponent would leave
        // lane 0 of the first signature, whose exponent is 0, out of whatever the compiler places around it)
        const uint32_t row0 = 512 * t + 8 * lane;
        w[0] = FP_ONE;
#pragma unroll 1
        for (int b = 20; b >= 0; b--) {
            w[0] = fp_sqr(w[0]);
            const fp ww = fp_mul(w[0], wn);
            w[0] = (row0 >> b) & 1 ? ww : w[0];
        }
#pragma unroll
        for (int r = 1; r < 8; r++) w[r] = fp_mul(w[r - 1], wn);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            dif[r] = x_sub(z, x_base<M>(w[r]));
            pre[r] = r ? x_mul(pre[r - 1], dif[r]) : dif[0];
        }
        Ext<M> inv = x_inv(pre[7]);
        static_down<7>([&](auto rc) { // indices known at compile time: the arrays stay in registers
            constexpr int r = decltype(rc)::value;
            Ext<M> term;
            if constexpr (r > 0) term = x_scale(x_mul(inv, pre[r - 1]), w[r]);
            else term = x_scale(inv, w[0]);
            inv = x_mul(inv, dif[r]);
            sum = x_add(sum, term);
            if (r == 0 && lane == 0) spec[wave][0] = term;
            if (r == 7 && lane < 4) spec[wave][1 + lane] = term;
            if (r == 7 && lane == 63) spec[wave][5] = term;
        });
    }
    red[wave][lane] = sum;
    __syncthreads();
    for (uint32_t s = 32; s > 0; s >>= 1) {
        if (lane < s) red[wave][lane] = x_add(red[wave][lane], red[wave][lane + s]);
        __syncthreads();
    }
    if (lane == 0) spec[wave][6] = red[wave][0];
    __syncthreads();
    if (lane < SCH_PUBLIC) {
        Ext<M> c = x_zero<M>();
        if (live) {
            const uint8_t *msg = buf + d.stmt + 8 * 28 * (size_t)t, *rx = buf + d.stmt + 8 * (28 * (size_t)T + 6 * (size_t)t);
            if (lane < 12) c = x_scale(spec[wave][6], ld64(msg + 8 * lane));
            else if (lane < 19) {
                for (uint32_t i = 0; i < 4; i++) c = x_add(c, x_scale(spec[wave][1 + i], ld64(msg + 8 * (lane - 12 + 7 * i))));
            } else if (lane < 25) c = x_scale(spec[wave][0], ld64(rx + 8 * (lane - 19)));
            else c = x_scale(spec[wave][5], ld64(rx + 8 * (lane - 25)));
        }
        contrib[wave][lane] = c;
    }
    __syncthreads();
    if (wave == 0 && lane < SCH_PUBLIC) {
        Ext<M> c = contrib[0][lane];
        for (uint32_t v = 1; v < SCH_TILE; v++) c = x_add(c, contrib[v][lane]);
        uint64_t *o = spub + d.sp + (size_t)M * (SCH_PUBLIC * blockIdx.x + lane);
        for (int q = 0; q < M; q++) o[q] = c.c[q];
    }
}
// One workgroup per proof of the group, lane v < 31: the tiles' partials added, times (z^n - 1) / n (v < 19) or
// (z^T w_512^(0 | 1) - 1) / T (the sequence values at step 0 | 511: w^(-511 T) = w_512) -> the values [31][M] behind the partials.
template <int M>
__global__ __launch_bounds__(64) void k_vfy_schnorr_public_sum(const VDesc *__restrict__ desc, const uint32_t *__restrict__ gp,
                                                               const uint64_t *__restrict__ tbase, uint64_t *__restrict__ spub) {
    const VDesc &d = desc[gp[blockIdx.x]];
    const uint32_t v = threadIdx.x, tiles = schnorr_tiles(d.n_sig);
    if (v >= SCH_PUBLIC) return;
    Ext<M> acc = x_zero<M>();
    for (uint32_t i = 0; i < tiles; i++) acc = x_add(acc, x_load<M>(spub + d.sp + (size_t)M * (SCH_PUBLIC * i + v)));
    Ext<M> zt = x_load<M>(tbase + d.tb + toff(d).z); // z^T, T = n / 512
    for (uint32_t s = 9; s < d.log_n; s++) zt = x_mul(zt, zt);
    Ext<M> f;
    uint64_t count;
    if (v < SCH_AUX) {
        f = zt;
        for (uint32_t s = 0; s < 9; s++) f = x_mul(f, f);
        count = 1ull << d.log_n;
    } else {
        f = v < SCH_AUX + 6 ? zt : x_scale(zt, fp_pow(d.k[K_WN], d.n_sig));
        count = d.n_sig;
    }
    f = x_scale(x_sub(f, x_one<M>()), fp_inv(fp_from_u64(count)));
    acc = x_mul(acc, f);
    uint64_t *o = spub + d.sp + (size_t)M * (SCH_PUBLIC * tiles + v);
    for (int q = 0; q < M; q++) o[q] = acc.c[q];
}

// Out-of-domain frames of the proofs gp[0..G) of one AIR (one workgroup each): periodic values at z^(n / cycle) from the proof's
// coefficient table in the cache (none for an AIR without periodic columns), then K frames t = 0..K-1 whose entries are e(t) = sum_q e_q t^q (K = 1 for m = 1); frame j of the group at
// column stride F.  bad[g] = 1 if an out-of-domain word is not below p.
template <int M>
__global__ __launch_bounds__(128) void k_vfy_ood_frames(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const uint32_t *__restrict__ gp,
                                                        const uint64_t *__restrict__ tbase, const uint64_t *__restrict__ pcoef, const uint64_t *__restrict__ spub,
                                                        uint32_t K, uint32_t F, fp *__restrict__ cur, fp *__restrict__ nxt, fp *__restrict__ per,
                                                        uint32_t *__restrict__ bad) {
    __shared__ Ext<M> pv[VMAX_NPER];
    const VDesc &d = desc[gp[blockIdx.x]];
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const uint32_t tid = threadIdx.x;
    bool ok = true;
    const uint32_t W = d.a.w, NP = d.a.nper + d.a.naux;
    for (uint32_t i = tid; i < (2 * W + d.a.ce) * M; i += 128) ok &= ld64(pb + d.ood + 8 * i) < FP_P;
    const int any_bad = __syncthreads_or(!ok);
    if (tid >= d.a.nper && tid < NP) // the statement's values at z (k_vfy_schnorr_public_sum)
        pv[tid] = x_load<M>(spub + d.sp + (size_t)M * (SCH_PUBLIC * schnorr_tiles(d.n_sig) + tid - d.a.nper));
    if (tid < d.a.nper) {
        Ext<M> zp = x_load<M>(tb + to.z);
        for (uint32_t s = d.a.log_cycle; s < d.log_n; s++) zp = x_mul(zp, zp);
        const uint32_t cycle = 1u << d.a.log_cycle;
        const uint64_t *co = pcoef + d.pcoef + (size_t)tid * cycle;
        Ext<M> acc = x_zero<M>();
        for (int i = (int)cycle - 1; i >= 0; i--) { acc = x_mul(acc, zp); acc.c[0] = fp_add(acc.c[0], co[i]); }
        pv[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) bad[blockIdx.x] = any_bad ? 1u : 0u;
    const uint32_t f0 = blockIdx.x * K;
    for (uint32_t e = tid; e < K * (2 * W + NP); e += 128) {
        const uint32_t t = e / (2 * W + NP), c = e % (2 * W + NP);
        Ext<M> v;
        fp *dst;
        if (c < W) { v = ld_ext<M>(pb + d.ood + 8 * M * c); dst = cur + (size_t)c * F; }
        else if (c < 2 * W) { v = ld_ext<M>(pb + d.ood + 8 * M * c); dst = nxt + (size_t)(c - W) * F; }
        else { v = pv[c - 2 * W]; dst = per + (size_t)(c - 2 * W) * F; }
        const fp tt = fp_from_u64(t);
        fp r = v.c[M - 1];
        for (int q = M - 2; q >= 0; q--) r = fp_add(fp_mul(r, tt), v.c[q]);
        dst[f0 + t] = r;
    }
}

template <int M> struct Lagrange { uint64_t w[18][M]; };

// One lane per proof of the group (one AIR, one extension degree): recombine the sampled constraint values, merge (transition divisor,
// degree adjustments, the AIR's single-row assertions) and compare with sum_i H_i z^i over the AIR's ce columns.
template <int M>
__global__ __launch_bounds__(64) void k_vfy_ood_check(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const uint32_t *__restrict__ gp,
                                                      uint32_t G, uint32_t K, uint32_t F, const fp *__restrict__ cvals, const uint32_t *__restrict__ bad,
                                                      Lagrange<M> lag, VGroups grps, VAsserts asr, const uint64_t *__restrict__ spub,
                                                      const uint64_t *__restrict__ tbase, uint32_t *__restrict__ slots) {
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= G) return;
    const VDesc &d = desc[gp[g]];
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const uint64_t *k = tb + to.k;
    const Ext<M> z = x_load<M>(tb + to.z);
    // constraint i's merge coefficient alpha_i + beta_i z^adj: the AIR's degree groups one after the other (z^adj in registers)
    Ext<M> acc = x_zero<M>();
#pragma unroll 1
    for (uint32_t grp = 0; grp < grps.n; grp++) {
        const Ext<M> za = x_pow(z, k[K_ADJ + grp]);
#pragma unroll 1
        for (uint32_t i = 0; i < d.a.nc; i++) {
            if (grps.g[i] != grp) continue;
            Ext<M> cv = x_zero<M>();
            for (uint32_t j = 0; j < K; j++) cv = x_add(cv, x_scale(x_load<M>(lag.w[j]), cvals[(size_t)i * F + g * K + j]));
            const Ext<M> coef = x_add(x_load<M>(tb + to.ta + M * i), x_mul(x_load<M>(tb + to.tb + M * i), za));
            acc = x_add(acc, x_mul(cv, coef));
        }
    }
    const fp w_last = k[K_WLAST];
    const Ext<M> one = x_one<M>();
    Ext<M> zn = z;
    for (uint32_t s = 0; s < d.log_n; s++) zn = x_mul(zn, zn);
    acc = x_mul(acc, x_mul(x_sub(z, x_base<M>(w_last)), x_inv(x_sub(zn, one))));
    const Ext<M> xb = x_pow(z, k[K_BADJ]);
    Ext<M> first = x_zero<M>(), last = x_zero<M>();
    Ext<M> d_first = x_sub(z, one), d_last = x_sub(z, x_base<M>(w_last));
    if (d.a.air == CSTARK_AIR_SCHNORR) {
        // 61 assertions on every 512th row from row 0 or row 511: divisors z^T - K_PUB[0 | 1] (= w_n^(first T)), values constant or the
        // statement's sequence values at z
        Ext<M> zt = z;
        for (uint32_t s = 9; s < d.log_n; s++) zt = x_mul(zt, zt);
        d_first = x_sub(zt, x_base<M>(k[K_PUB]));
        d_last = x_sub(zt, x_base<M>(k[K_PUB + 1]));
        const uint64_t *sv = spub + d.sp + (size_t)M * (SCH_PUBLIC * schnorr_tiles(d.n_sig) + SCH_AUX);
#pragma unroll 1
        for (uint32_t a = 0; a < asr.n; a++) {
            const Ext<M> c = ld_ext<M>(pb + d.ood + 8 * M * asr.reg[a]);
            const uint32_t vk = asr.val[a];
            const Ext<M> val = vk >= 2 ? x_load<M>(sv + M * (vk - 2)) : vk ? one : x_zero<M>();
            const Ext<M> term = x_mul(x_sub(c, val), x_add(x_load<M>(tb + to.ba + M * a), x_mul(x_load<M>(tb + to.bb + M * a), xb)));
            if (asr.div[a]) last = x_add(last, term);
            else first = x_add(first, term);
        }
    }
    const uint32_t hn = d.a.air == CSTARK_AIR_SCHNORR ? 0 : d.a.na / 2;
#pragma unroll 1
    for (uint32_t a = 0; a < hn; a++) {
        const Ext<M> c = ld_ext<M>(pb + d.ood + 8 * M * (d.a.areg + a));
        first = x_add(first, x_mul(x_sub(c, x_base<M>(k[K_PUB + a])), x_add(x_load<M>(tb + to.ba + M * a), x_mul(x_load<M>(tb + to.bb + M * a), xb))));
        last = x_add(last, x_mul(x_sub(c, x_base<M>(k[K_PUB + hn + a])),
                                 x_add(x_load<M>(tb + to.ba + M * (hn + a)), x_mul(x_load<M>(tb + to.bb + M * (hn + a)), xb))));
    }
    const Ext<M> lhs = x_add(acc, x_add(x_mul(first, x_inv(d_first)), x_mul(last, x_inv(d_last))));
    Ext<M> rhs = x_zero<M>(), zi = one;
    for (uint32_t i = 0; i < d.a.ce; i++) {
        rhs = x_add(rhs, x_mul(ld_ext<M>(pb + d.ood + 8 * M * (2 * d.a.w + i)), zi));
        zi = x_mul(zi, z);
    }
    slots[d.slot0] = bad[g] ? (uint32_t)RK_MALFORMED : x_eq(lhs, rhs) ? (uint32_t)RK_NONE : (uint32_t)RK_OOD;
}

// One lane per (proof, query): DEEP value at x = g w_N^pos, then every layer -- the value against the opened row, the fold of the row
// -- and finally the remainder (a proof without a layer: the DEEP value against the remainder directly).  Slots and positions come from the host's replay and were checked against the layer's row count.
template <int M>
__global__ __launch_bounds__(128) void k_vfy_fri(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const uint32_t *__restrict__ gp,
                                                 const uint64_t *__restrict__ tbase, uint32_t *__restrict__ slots) {
    const VDesc &d = desc[gp[blockIdx.y]]; // read in place: lrows[] is indexed by the layer
    const uint32_t q = blockIdx.x * 128 + threadIdx.x;
    if (q >= d.nq) return;
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const uint64_t *k = tb + to.k;
    uint32_t pos = (uint32_t)tb[to.pos + q];
    const fp g = k[K_G];
    fp x = fp_mul(g, fp_pow(k[K_WNN], pos));
    const Ext<M> z = x_load<M>(tb + to.z);
    const Ext<M> zw = x_scale(z, k[K_WN]);
    Ext<M> zb = z;
    for (uint32_t s = 1; s < d.a.ce; s <<= 1) zb = x_mul(zb, zb); // z^ce: the composition columns
    const uint32_t W = d.a.w, CE = d.a.ce;
    Ext<M> s1 = x_zero<M>(), s2 = x_zero<M>(), s3 = x_zero<M>();
    const uint8_t *row = pb + d.trows + 8 * (size_t)q * W;
    for (uint32_t c = 0; c < W; c++) {
        const Ext<M> rv = x_base<M>(ld64(row + 8 * c));
        s1 = x_add(s1, x_mul(x_load<M>(tb + to.da + M * c), x_sub(rv, ld_ext<M>(pb + d.ood + 8 * M * c))));
        s2 = x_add(s2, x_mul(x_load<M>(tb + to.db + M * c), x_sub(rv, ld_ext<M>(pb + d.ood + 8 * M * (W + c)))));
    }
    const uint8_t *crow = pb + d.crows + 8 * (size_t)q * CE * M;
    for (uint32_t i = 0; i < CE; i++)
        s3 = x_add(s3, x_mul(x_load<M>(tb + to.dd + M * i), x_sub(ld_ext<M>(crow + 8 * M * i), ld_ext<M>(pb + d.ood + 8 * M * (2 * W + i)))));
    const Ext<M> bx = x_base<M>(x);
    const Ext<M> t = x_add(x_add(x_mul(s1, x_inv(x_sub(bx, z))), x_mul(s2, x_inv(x_sub(bx, zw)))), x_mul(s3, x_inv(x_sub(bx, zb))));
    Ext<M> val = x_mul(t, x_add(x_load<M>(tb + to.dga), x_scale(x_load<M>(tb + to.dgb), x)));

    const uint32_t f = 1u << d.log_f;
    fp offset = g;
    uint32_t lgl = d.log_N, rank = RK_NONE;
    for (uint32_t l = 0; l < d.n_layers && rank == RK_NONE; l++) {
        if (l >= (uint32_t)tb[to.st]) { slots[d.slot0 + 1 + d.n_open + q] = RK_NONE; return; } // the replay reported LAYER_COUNT(l)
        const uint32_t lr = lgl - d.log_f, slot = (uint32_t)tb[to.slot + l * d.nq + q];
        const uint8_t *lrow = pb + d.lrows[l] + 8 * (size_t)slot * f * M;
        const uint32_t kk = pos >> lr;
        Ext<M> v;
        for (int c = 0; c < M; c++) v.c[c] = ld64(lrow + 8 * ((size_t)f * c + kk));
        if (!x_eq(v, val)) { rank = RK_LAYER0 + 3 * l + 2; break; }
        const uint32_t rp = pos & ((1u << lr) - 1);
        const fp xl = fp_mul(offset, fp_pow(k[K_WL + l], rp));
        const Ext<M> r = x_scale(x_load<M>(tb + to.alpha + M * l), fp_inv(xl));
        Ext<M> acc = x_zero<M>(), rs = x_one<M>();
        fp zs = FP_ONE; // zeta^-s
        for (uint32_t s = 0; s < f; s++) {
            Ext<M> cs = x_zero<M>();
            fp w = FP_ONE; // zeta^-(s j)
            for (uint32_t j = 0; j < f; j++) {
                Ext<M> e;
                for (int c = 0; c < M; c++) e.c[c] = ld64(lrow + 8 * ((size_t)f * c + j));
                cs = x_add(cs, x_scale(e, w));
                w = fp_mul(w, zs);
            }
            acc = x_add(acc, x_mul(x_scale(cs, k[K_INVF]), rs));
            rs = x_mul(rs, r);
            zs = fp_mul(zs, k[K_ZETA_INV]);
        }
        val = acc;
        pos = rp;
        for (uint32_t s = 0; s < d.log_f; s++) offset = fp_sqr(offset);
        lgl = lr;
    }
    if (rank == RK_NONE) {
        Ext<M> rv;
        for (int c = 0; c < M; c++) rv.c[c] = ld64(pb + d.rem + 8 * ((size_t)c * d.R + pos));
        if (!x_eq(rv, val)) rank = RK_REMAINDER_FOLDING;
    }
    slots[d.slot0 + 1 + d.n_open + q] = rank;
}

// One workgroup per (proof, remainder component): every word below p, and the coefficients of degree >= R / blowup of the inverse
// transform all zero (evaluations over offset * <w_R>: the offset does not change which coefficients vanish).
__global__ __launch_bounds__(256) void k_vfy_remainder(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, const uint64_t *__restrict__ tbase,
                                                       uint32_t *__restrict__ slots) {
    __shared__ fp v[1024], wt[1024];
    const VDesc &d = desc[blockIdx.y];
    const uint32_t comp = blockIdx.x;
    if (comp >= d.m) return;
    const uint8_t *pb = buf + d.base;
    const uint64_t *tb = tbase + d.tb;
    const TOff to = toff(d);
    const fp wrinv = tb[to.k + K_WRINV];
    const uint32_t R = d.R;
    bool ok = true;
    for (uint32_t j = threadIdx.x; j < R; j += 256) {
        const fp e = ld64(pb + d.rem + 8 * ((size_t)comp * R + j));
        ok &= e < FP_P;
        v[j] = e;
        wt[j] = fp_pow(wrinv, j);
    }
    const int any_bad = __syncthreads_or(!ok);
    bool high = false;
    if (!any_bad)
        for (uint32_t c = (R >> d.log_b) + threadIdx.x; c < R; c += 256) {
            fp s = 0;
            for (uint32_t j = 0; j < R; j++) s = fp_add(s, fp_mul(v[j], wt[(j * c) & (R - 1)]));
            high |= s != 0;
        }
    const int any_high = __syncthreads_or(high);
    if (threadIdx.x == 0)
        slots[d.slot0 + 1 + d.n_open + d.nq + comp] = any_bad ? (uint32_t)RK_MALFORMED : any_high ? (uint32_t)RK_REMAINDER_DEGREE : (uint32_t)RK_NONE;
}

__device__ __forceinline__ int32_t rank_verdict(uint32_t r) {
    if (r == RK_NONE) return CSTARK_PROOF_OK;
    if (r == RK_MALFORMED) return CSTARK_PROOF_MALFORMED;
    if (r == RK_OOD) return CSTARK_PROOF_OOD;
    if (r == RK_REMAINDER_COMMITMENT) return CSTARK_PROOF_REMAINDER_COMMITMENT;
    if (r == RK_POW) return CSTARK_PROOF_POW;
    if (r < RK_LAYER0) return ((r - RK_OPENING0) & 1) ? CSTARK_PROOF_COMPOSITION_OPENING : CSTARK_PROOF_TRACE_OPENING;
    if (r < RK_REMAINDER_FOLDING) return CSTARK_PROOF_LAYER_COUNT + (int32_t)((r - RK_LAYER0) % 3);
    return r == RK_REMAINDER_FOLDING ? CSTARK_PROOF_REMAINDER_FOLDING : CSTARK_PROOF_REMAINDER_DEGREE;
}
// one workgroup per proof: the smallest rank among its slots and the replay's
__global__ __launch_bounds__(256) void k_vfy_reduce(const VDesc *__restrict__ desc, const uint64_t *__restrict__ tbase, const uint32_t *__restrict__ slots,
                                                    int32_t *__restrict__ verdicts) {
    __shared__ uint32_t red[256];
    const VDesc &d = desc[blockIdx.x];
    const uint32_t n = 1 + d.n_open + d.nq + d.m;
    uint32_t r = threadIdx.x == 0 ? (uint32_t)tbase[d.tb + toff(d).st + 1] : RK_NONE;
    for (uint32_t i = threadIdx.x; i < n; i += 256) r = min(r, slots[d.slot0 + i]);
    red[threadIdx.x] = r;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) verdicts[blockIdx.x] = rank_verdict(red[0]);
}


// ---- transcript replay on the device ----------------------------------------------------------------------------------------------
// The prover's coin (coin.h) in one workgroup per proof.  Thread 0 walks the reseed chain; the draws that follow one seed are
// independent, so the 256 lanes hash 256 consecutive counters at once and thread 0 takes the accepted candidates in counter order.
constexpr int VT = 256;
// the hash routines as calls: inlined at every use in one kernel they exceed the register file
__device__ __noinline__ void nb3_chunk(const uint8_t *p, uint32_t len, uint64_t chunk, bool root, uint32_t (&cv)[8]) { vh::b3_chunk(p, len, chunk, root, cv); }
__device__ __noinline__ void nb3_merge(uint32_t (*cvs)[8], uint32_t n, uint32_t (&out)[8]) { vh::b3_merge(cvs, n, out); }
__device__ __noinline__ void nsha3(const uint8_t *p, uint32_t len, uint64_t (&out)[4]) { vh::sha3(p, len, out); }
struct TShared {
    uint8_t msg[160];          // the seed message: context || public inputs (129 bytes)
    uint32_t seed[8];
    uint32_t dig[8];
    uint64_t cand[VT];
    uint32_t flag[VT];
    uint32_t cvs[32][8];       // chunk chaining values of one multi-chunk Blake3 message (at most 32 KB: the cubic remainder is 24 KB)
    uint32_t pos[128], lpos[128];
    uint64_t counter;
    uint32_t got, ok_layers, rank, n_lpos;
};
// H(a[0..8) || b) for a 32-byte b given as eight words, or as one 64-bit integer (nb = 2 words): the coin's two message shapes
__device__ __noinline__ void coin_hash(uint32_t hash, const uint32_t *a, const uint32_t *b, uint32_t nb, uint32_t (&out)[8]) {
    if (hash == 1) {
        uint64_t st[25];
#pragma unroll
        for (int i = 0; i < 25; i++) st[i] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) st[i] = (uint64_t)a[2 * i] | ((uint64_t)a[2 * i + 1] << 32);
        if (nb == 8) {
#pragma unroll
            for (int i = 0; i < 4; i++) st[4 + i] = (uint64_t)b[2 * i] | ((uint64_t)b[2 * i + 1] << 32);
            st[8] ^= 0x06;
        } else {
            st[4] = (uint64_t)b[0] | ((uint64_t)b[1] << 32);
            st[5] ^= 0x06;
        }
        st[16] ^= 0x80ull << 56;
        keccak::permute(st);
#pragma unroll
        for (int i = 0; i < 4; i++) { out[2 * i] = (uint32_t)st[i]; out[2 * i + 1] = (uint32_t)(st[i] >> 32); }
    } else {
        uint32_t mw[16];
#pragma unroll
        for (int i = 0; i < 8; i++) { mw[i] = a[i]; mw[8 + i] = (nb == 8 || i < 2) ? b[i] : 0u; out[i] = vh::iv(i); }
        vh::compress(out, mw, 0, 4 * (8 + nb), vh::B3_CHUNK_START | vh::B3_CHUNK_END | vh::B3_ROOT);
    }
}
__device__ __forceinline__ uint64_t first_u64(const uint32_t (&h)[8]) { return (uint64_t)h[0] | ((uint64_t)h[1] << 32); }
__device__ __forceinline__ void with_int(uint32_t hash, const uint32_t *seed, uint64_t v, uint32_t (&out)[8]) {
    const uint32_t w[8] = {(uint32_t)v, (uint32_t)(v >> 32), 0, 0, 0, 0, 0, 0};
    coin_hash(hash, seed, w, 2, out);
}
// digest of len bytes at p into sh.dig (all threads call; Blake3 chunks in parallel, then thread 0 merges)
__device__ void block_digest(uint32_t hash, const uint8_t *p, uint32_t len, TShared &sh) {
    const uint32_t n = len <= 1024 ? 1 : (len + 1023) / 1024;
    if (hash == 0 && n > 1) {
        for (uint32_t c = threadIdx.x; c < n; c += VT) {
            uint32_t cv[8];
            nb3_chunk(p + 1024 * (size_t)c, len - 1024 * c < 1024 ? len - 1024 * c : 1024, c, false, cv);
            for (int k = 0; k < 8; k++) sh.cvs[c][k] = cv[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (hash == 1) {
            uint64_t h[4];
            nsha3(p, len, h);
            for (int i = 0; i < 4; i++) { sh.dig[2 * i] = (uint32_t)h[i]; sh.dig[2 * i + 1] = (uint32_t)(h[i] >> 32); }
        } else {
            uint32_t h[8];
            if (n == 1) nb3_chunk(p, len, 0, true, h);
            else nb3_merge(sh.cvs, n, h);
            for (int i = 0; i < 8; i++) sh.dig[i] = h[i];
        }
    }
    __syncthreads();
}
// seed <- H(seed || d), d 32 bytes at a 4-aligned address (thread 0)
__device__ void reseed(uint32_t hash, TShared &sh, const uint32_t *d) {
    uint32_t h[8];
    coin_hash(hash, sh.seed, d, 8, h);
    for (int i = 0; i < 8; i++) sh.seed[i] = h[i];
    sh.counter = CSTARK_CONV_COIN_FIRST_COUNTER - 1;
}
__device__ __forceinline__ const uint32_t *w32(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
// `count` field elements (memory form) in draw order; put(i, v) runs on thread 0
template <class Put> __device__ void draws(uint32_t hash, TShared &sh, uint32_t count, Put put) {
    if (threadIdx.x == 0) sh.got = 0;
    __syncthreads();
    while (sh.got < count) {
        uint32_t h[8];
        with_int(hash, sh.seed, sh.counter + 1 + threadIdx.x, h);
        sh.cand[threadIdx.x] = first_u64(h);
        __syncthreads();
        if (threadIdx.x == 0)
            for (int t = 0; t < VT && sh.got < count; t++) {
                sh.counter++;
                const uint64_t v = sh.cand[t];
                if (!CSTARK_CONV_COIN_REJECT_ABOVE_P || v < FP_P) put(sh.got++, fp_from_u64(v));
            }
        __syncthreads();
    }
}
// distinct values of (list & (rows - 1)) in first-occurrence order, list[0..n) -> sh.lpos, count -> sh.n_lpos (all threads call)
__device__ void fold_list(TShared &sh, const uint32_t *list, uint32_t n, uint32_t rows) {
    const uint32_t i = threadIdx.x;
    if (i < n) {
        const uint32_t r = list[i] & (rows - 1);
        bool first = true;
        for (uint32_t j = 0; j < i; j++) first &= (list[j] & (rows - 1)) != r;
        sh.flag[i] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < n; j++) if (sh.flag[j]) sh.cand[c++] = list[j] & (rows - 1);
        sh.n_lpos = c;
    }
    __syncthreads();
    if (i < sh.n_lpos) sh.lpos[i] = (uint32_t)sh.cand[i];
    __syncthreads();
}

__global__ __launch_bounds__(VT) void k_vfy_transcript(const uint8_t *__restrict__ buf, const VDesc *__restrict__ desc, uint64_t *__restrict__ tbase) {
    __shared__ TShared sh;
    const VDesc &d = desc[blockIdx.x];
    const uint8_t *pb = buf + d.base;
    uint64_t *T = tbase + d.tb;
    const uint32_t m = d.m, nq = d.nq, nl = d.n_layers, hash = d.hash, tid = threadIdx.x;
    const uint32_t W = d.a.w, CE = d.a.ce, NC = d.a.nc, NA = d.a.na;
    const TOff to = toff(d);
    for (uint32_t i = tid; i < K_WORDS; i += VT) T[to.k + i] = d.k[i];
    if (tid == 0) {
        // seed = H(width, log n | p | nq, log b, grinding, hash, extension, folding, log remainder | the AIR's public inputs, canonical)
        uint32_t o = 0;
        sh.msg[o++] = (uint8_t)W; sh.msg[o++] = (uint8_t)d.log_n;
        for (int i = 0; i < 8; i++) sh.msg[o++] = (uint8_t)(FP_P >> (8 * i));
        const uint32_t ob[7] = {nq, d.log_b, d.grinding, hash, m - 1, 1u << d.log_f, d.log_rem};
        for (int i = 0; i < 7; i++) sh.msg[o++] = (uint8_t)ob[i];
        for (uint32_t i = 0; i < d.a.npub; i++) {
            const uint64_t v = fp_to_u64(d.pub[i]);
            for (int k = 0; k < 8; k++) sh.msg[o++] = (uint8_t)(v >> (8 * k));
        }
        if (d.a.npub == 0) { // a statement too long for sh.msg (SchnorrAir): the host hashed the seed message
            for (int i = 0; i < 8; i++) sh.seed[i] = d.seed[i];
        } else if (hash == 1) {
            uint64_t h[4];
            nsha3(sh.msg, o, h);
            for (int i = 0; i < 4; i++) { sh.seed[2 * i] = (uint32_t)h[i]; sh.seed[2 * i + 1] = (uint32_t)(h[i] >> 32); }
        } else {
            uint32_t h[8];
            nb3_chunk(sh.msg, o, 0, true, h);
            for (int i = 0; i < 8; i++) sh.seed[i] = h[i];
        }
        reseed(hash, sh, w32(pb + 52)); // trace root
        sh.rank = RK_NONE;
    }
    __syncthreads();
    // (alpha, beta) per constraint, then per assertion: elements of E (m draws each)
    draws(hash, sh, 2 * (NC + NA) * m, [&](uint32_t i, uint64_t v) {
        const uint32_t e = i / m, q = i % m, pair = e / 2, which = e % 2;
        if (pair < NC) T[(which ? to.tb : to.ta) + m * pair + q] = v;
        else T[(which ? to.bb : to.ba) + m * (pair - NC) + q] = v;
    });
    if (tid == 0) reseed(hash, sh, w32(pb + 84)); // constraint root
    __syncthreads();
    draws(hash, sh, m, [&](uint32_t i, uint64_t v) { T[to.z + i] = v; });
    block_digest(hash, pb + d.ood, 8 * 2 * W * m, sh);
    if (tid == 0) reseed(hash, sh, sh.dig);
    __syncthreads();
    block_digest(hash, pb + d.ood + 8 * 2 * W * m, 8 * CE * m, sh);
    if (tid == 0) reseed(hash, sh, sh.dig);
    __syncthreads();
    constexpr uint32_t PER = CSTARK_CONV_DEEP_DRAWS_PER_REGISTER;
    draws(hash, sh, (W * PER + CE + 2) * m, [&](uint32_t i, uint64_t v) {
        const uint32_t e = i / m, q = i % m;
        if (e < W * PER) {
            const uint32_t c = e / PER, k = e % PER;
            if (k == 0) T[to.da + m * c + q] = v;
            else if (k == 1) T[to.db + m * c + q] = v;
        } else {
            const uint32_t e2 = e - W * PER;
            if (e2 < CE) T[to.dd + m * e2 + q] = v;
            else if (e2 == CE) T[to.dga + q] = v;
            else T[to.dgb + q] = v;
        }
    });
    for (uint32_t l = 0; l < nl; l++) {
        if (tid == 0) reseed(hash, sh, w32(pb + 120 + 32 * l));
        __syncthreads();
        draws(hash, sh, m, [&](uint32_t i, uint64_t v) { T[to.alpha + m * l + i] = v; });
    }
    const uint8_t *rem_commit = pb + 120 + 32 * nl;
    block_digest(hash, pb + d.rem, 8 * d.R * m, sh);
    if (tid == 0) {
        const uint32_t *rc = w32(rem_commit);
        bool same = true;
        for (int i = 0; i < 8; i++) same &= sh.dig[i] == rc[i];
        if (!same) sh.rank = RK_REMAINDER_COMMITMENT;
        reseed(hash, sh, rc);
        const uint32_t *nw = w32(pb + d.ood + 8 * (2 * W + CE) * m);
        const uint64_t nonce = (uint64_t)nw[0] | ((uint64_t)nw[1] << 32);
        uint32_t h[8];
        with_int(hash, sh.seed, nonce, h);
        if (d.grinding && (first_u64(h) & ((1ull << d.grinding) - 1)) && sh.rank == RK_NONE) sh.rank = RK_POW;
        for (int i = 0; i < 8; i++) sh.seed[i] = h[i]; // reseed_int(nonce)
        sh.counter = CSTARK_CONV_COIN_FIRST_COUNTER - 1;
        sh.got = 0;
    }
    __syncthreads();
    // query positions: nq distinct integers below N (duplicates skipped: CSTARK_CONV_QUERY_DEDUP)
    const uint32_t Nmask = (1u << d.log_N) - 1;
    while (sh.got < nq) {
        uint32_t h[8];
        with_int(hash, sh.seed, sh.counter + 1 + tid, h);
        const uint32_t v = (uint32_t)(first_u64(h) & Nmask);
        sh.cand[tid] = v;
        __syncthreads();
        bool fresh = true;
        if (CSTARK_CONV_QUERY_DEDUP) {
            for (uint32_t j = 0; j < sh.got; j++) fresh &= sh.pos[j] != v;
            for (uint32_t j = 0; j < tid; j++) fresh &= (uint32_t)sh.cand[j] != v;
        }
        sh.flag[tid] = fresh;
        __syncthreads();
        if (tid == 0)
            for (int t = 0; t < VT && sh.got < nq; t++) {
                sh.counter++;
                if (sh.flag[t]) sh.pos[sh.got++] = (uint32_t)sh.cand[t];
            }
        __syncthreads();
    }
    for (uint32_t q = tid; q < nq; q += VT) T[to.pos + q] = sh.pos[q];
    // folded positions of every layer and the row slot of each query, up to the first layer whose stated count differs
    if (tid == 0) sh.ok_layers = nl;
    __syncthreads();
    uint32_t lg = d.log_N, prev_n = nq;
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t rows = 1u << (lg - d.log_f);
        fold_list(sh, l == 0 ? sh.pos : sh.lpos, prev_n, rows);
        if (sh.n_lpos != d.npos[l]) {
            if (tid == 0) { sh.ok_layers = l; sh.rank = min(sh.rank, RK_LAYER0 + 3 * l); }
            break;
        }
        for (uint32_t t = tid; t < sh.n_lpos; t += VT) T[to.lpos + l * nq + t] = sh.lpos[t];
        for (uint32_t q = tid; q < nq; q += VT) {
            const uint32_t r = sh.pos[q] & (rows - 1);
            uint32_t slot = 0;
            for (uint32_t j = 0; j < sh.n_lpos; j++) if (sh.lpos[j] == r) slot = j;
            T[to.slot + l * nq + q] = slot;
        }
        prev_n = sh.n_lpos;
        lg -= d.log_f;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) { T[to.st] = sh.ok_layers; T[to.st + 1] = sh.rank; }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
constexpr size_t VFY_CHUNK_BYTES = CSTARK_VERIFY_CHUNK_BYTES; // staging budget of one chunk (cstark.h)
constexpr size_t SCH_STATEMENT_BYTES = 8 * 34 + 32;          // one signature of SchnorrAir's statement: message, R.x, s
enum { VFY_EVENTS = CSTARK_VERIFY_NUM_STAGES };

struct VerifyArena {
    uint8_t *h_stage = nullptr, *d_stage = nullptr;
    size_t stage_bytes = 0;
    void *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    int32_t *h_verdicts = nullptr;
    size_t verdict_cap = 0;
    // periodic coefficients per (AIR, header word): TransactionAir [depth slot][48][1024], depth = 2^(slot+1) - 1 | MerkleAir
    // [depth slot][33][512] | RescueAir [29][8] | SchnorrAir [36][512]
    uint64_t *d_pcoef = nullptr;
    bool pcoef_ready[14] = {};
    struct Adj { uint32_t air, log_n; uint64_t adj[VMAX_GROUPS], badj, zc[2]; }; // zc: SchnorrAir's two assertion divisors x^(n / 512) - zc
    std::vector<Adj> adj;                  // degree adjustments per (AIR, log_n): the constraint-evaluation domain is n * ce (SchnorrAir:
                                           // log_n == 9 is the one-signature shape, whose bit constraints have a lower degree)
    hipEvent_t ev[VFY_EVENTS] = {};
    float ms[CSTARK_VERIFY_NUM_STAGES] = {};
    uint64_t h2d_bytes = 0;              // bytes copied host -> device by the last verify call
    bool timed = false;
    uint8_t *h_out = nullptr;            // convert calls: the new path sections of a chunk, copied back (pinned)
    size_t out_bytes = 0;
};

void verify_arena_free(VerifyArena *a) {
    if (!a) return;
    if (a->h_stage) (void)hipHostFree(a->h_stage);
    if (a->d_stage) (void)hipFree(a->d_stage);
    if (a->d_scratch) (void)hipFree(a->d_scratch);
    if (a->h_verdicts) (void)hipHostFree(a->h_verdicts);
    if (a->h_out) (void)hipHostFree(a->h_out);
    if (a->d_pcoef) (void)hipFree(a->d_pcoef);
    for (hipEvent_t e : a->ev) if (e) (void)hipEventDestroy(e);
    delete a;
}

namespace {

struct Staged {
    uint32_t index;     // position in the caller's arrays
    const uint8_t *bytes;
    const cstark_schnorr_statement *stm = nullptr; // SchnorrAir: the caller's statement (n_sig equals the header's)
    Layout L;
    VDesc d;
    uint32_t D;         // the AIR's largest constraint degree (AirInfo)
    size_t out_at[MAX_TREES] = {}; // convert calls, a proof that changes its form: where tree t's new section lies in the output block
    uint32_t count_at = 0;         // ... to the compact form: its trees' node counts are counts[count_at + t]
};
// What a convert call adds to a verify call: the target form and the caller's buffers (verify_batch has checked the capacities).
struct Convert { uint32_t form; uint8_t *const *out; const size_t *capacities; size_t *out_lens; };
// the proofs of one (AIR, extension degree) of a chunk: their list, the frames sampled for them (K each) and the constraint values
struct Group {
    uint32_t start = 0, count = 0, K = 0, frames = 0, tiles = 0; // tiles: SchnorrAir, those of the group's largest statement
    fp *cur, *nxt, *per, *val;
    uint32_t *bad;
};

// The AIRs the pipeline verifies, as data, built once per process.  D: the largest total degree of a constraint in the frame's entries
// (trace registers and periodic values), the sum of cstark_air_constraint_degree's two answers.  groups: constraints of one degree
// (base; cycles) share an adjustment exponent at every trace length, so the grouping is the AIR's own; rep[g] = a constraint of group g.
// SchnorrAir: `shape` is the one-signature shape, whose grouping is the finer one (the bit constraints 19..36 are a group of their own;
// from two signatures on they have the degree of constraints 0..5, and the two groups then carry the same exponent), shape_many the
// shape from two signatures on; asserts lists its 61 assertions.
struct AirInfo {
    bool ok = false; VAir a{}; uint32_t D = 0; VGroups groups{}; uint32_t rep[VMAX_GROUPS] = {}; host::AirShape shape, shape_many; VAsserts asserts{};
};
const AirInfo &air_info(uint32_t air) {
    static const std::array<AirInfo, 5> table = [] {
        std::array<AirInfo, 5> t;
        for (uint32_t id = 0; id < 5; id++) {
            AirInfo &I = t[id];
            if (id == CSTARK_AIR_STATE_TRANSITION) {
                I.ok = true;
                I.a = {id, AIR_WIDTH[id], AIR_CE[id], 115, 4, 14, host::TX_NUM_PERIODIC, 10, 58};
                I.D = 7;
                I.groups.n = 5;
                for (uint32_t i = 0; i < I.a.nc; i++) I.groups.g[i] = (uint8_t)tx_degree_group((int)i);
                continue;
            }
            host::AirShape &s = I.shape;
            if (!host::air_shape((int)id, s, 1)) continue;
            I.ok = true;
            I.a = {id, s.width, 1u << s.log_ce_blowup(), s.n_constraints, (uint32_t)s.a_reg.size(),
                   id == CSTARK_AIR_RANGE ? 1u : id == CSTARK_AIR_SCHNORR ? 0u : 14u, s.n_periodic, s.cycle_len ? ilog2(s.cycle_len) : 0, s.a_reg[0], 0};
            if (id == CSTARK_AIR_SCHNORR) {
                host::air_shape((int)id, I.shape_many, 2);
                I.a.naux = SCH_AUX;
                assert(s.a_reg.size() == VMAX_NA);
                I.asserts.n = (uint8_t)s.a_reg.size();
                for (size_t a = 0; a < s.a_reg.size(); a++) {
                    assert(s.a_stride[a] == 512 && (s.a_first[a] == 0 || s.a_first[a] == 511) && (s.a_const[a] == 0 || s.a_const[a] == host::ONE));
                    I.asserts.reg[a] = (uint8_t)s.a_reg[a];
                    I.asserts.div[a] = s.a_first[a] ? 1 : 0;
                    I.asserts.val[a] = s.a_seq[a] >= 0 ? (uint8_t)(2 + s.a_seq[a]) : s.a_const[a] ? 1 : 0;
                }
            }
            for (uint32_t i = 0; i < s.n_constraints; i++) {
                I.D = std::max(I.D, s.base[i] + (s.cycle_len ? s.cycles[i] : 0)); // (SchnorrAir: 7 in either shape)
                uint32_t g = 0;
                while (g < I.groups.n && !(s.base[I.rep[g]] == s.base[i] && s.cycles[I.rep[g]] == s.cycles[i])) g++;
                if (g == I.groups.n) { assert(g < VMAX_GROUPS); I.rep[I.groups.n++] = i; }
                I.groups.g[i] = (uint8_t)g;
            }
        }
        return t;
    }();
    return table[air];
}
// header values no prover of this library writes (cstark_tx_witness_upload, cstark_air_prove, cstark_range_prove_bits,
// cstark_rescue_prove, prove.hip): checked before anything is sized or cached from them
bool header_ok(const Layout &L) {
    if (L.nq > (1u << L.log_N) / 2) return false;
    switch (L.air) {
    case CSTARK_AIR_STATE_TRANSITION: return L.log_n >= 10 && tx_depth_ok(L.word);
    case CSTARK_AIR_MERKLE_UPDATE: return L.log_n >= 9 && tx_depth_ok(L.word);
    case CSTARK_AIR_RANGE: return L.word == 0; // log_n in 6 .. 21: parse_layout
    case CSTARK_AIR_RESCUE_CHAIN: return L.word == 1u << (L.log_n - 3); // the chain length; log_n in 6 .. 21: parse_layout
    case CSTARK_AIR_SCHNORR: return L.log_n >= 9 && L.word == 1u << (L.log_n - 9); // the number of signatures, 512 rows each
    }
    return false;
}

// degree adjustments of (AIR, log_n), one per constraint group: TransactionAir's own five (air_tx_host.h), the sub-AIRs' from air_groups.h
const VerifyArena::Adj &adjustments(VerifyArena *a, const AirInfo &I, uint32_t log_n) {
    for (const VerifyArena::Adj &e : a->adj)
        if (e.air == I.a.air && e.log_n == log_n) return e;
    using namespace host;
    const uint64_t n = 1ull << log_n;
    VerifyArena::Adj e{I.a.air, log_n, {}, 0, {}};
    if (I.a.air == CSTARK_AIR_STATE_TRANSITION) {
        for (int g = 0; g < 5; g++) e.adj[g] = tx_group_adjustment(g, n, n * I.a.ce);
        e.badj = tx_boundary_adjustment(n, n * I.a.ce);
    } else {
        AirGroups q;
        const AirShape &shape = I.a.air == CSTARK_AIR_SCHNORR && log_n > 9 ? I.shape_many : I.shape;
        const AirGroupsResult r = air_groups(shape, log_n, 0, q); // at most as many distinct exponents as degrees: air_info's bound
        assert(r == AIR_GROUPS_OK);
        (void)r;
        for (uint32_t g = 0; g < I.groups.n; g++) e.adj[g] = q.tgrp_adj[q.t_grp[I.rep[g]]];
        e.badj = q.agrp_badj[0]; // single-row assertions only: one adjustment (SchnorrAir: both divisors have n / 512 steps)
        if (I.a.air == CSTARK_AIR_SCHNORR) { assert(q.n_agrp == 2 && q.agrp_badj[1] == e.badj); e.zc[0] = q.agrp_zc[0]; e.zc[1] = q.agrp_zc[1]; }
    }
    a->adj.push_back(e);
    return a->adj.back();
}

// what the device needs besides the proof bytes: the AIR, the domain constants and the public inputs (the transcript itself is replayed
// on the device, k_vfy_transcript).  pub: the caller's 14 words (RangeProofAir: word 0 = number).
void describe(const Layout &L, const AirInfo &I, const VerifyArena::Adj &adj, const uint64_t *pub, VDesc &d) {
    using namespace host;
    const uint64_t n = 1ull << L.log_n;
    uint64_t *K = d.k;
    d.a = I.a;
    K[K_WN] = root_of_unity(L.log_n);
    K[K_WNN] = root_of_unity(L.log_N);
    K[K_WLAST] = pow(K[K_WN], n - 1);
    K[K_G] = lde_offset();
    for (uint32_t g = 0; g < VMAX_GROUPS; g++) K[K_ADJ + g] = adj.adj[g];
    K[K_BADJ] = adj.badj;
    K[K_INVF] = inv(from_u64(L.f));
    K[K_ZETA_INV] = inv(root_of_unity(L.log_f));
    K[K_WRINV] = inv(root_of_unity(ilog2(L.R)));
    // asserted values: the first na / 2 at row 0, the others at row n - 1
    if (L.air == CSTARK_AIR_STATE_TRANSITION) { K[K_PUB] = pub[0]; K[K_PUB + 1] = pub[1]; K[K_PUB + 2] = pub[7]; K[K_PUB + 3] = pub[8]; }
    else if (L.air == CSTARK_AIR_RANGE) { K[K_PUB] = 0; K[K_PUB + 1] = pub[0]; }
    else if (L.air == CSTARK_AIR_SCHNORR) { K[K_PUB] = adj.zc[0]; K[K_PUB + 1] = adj.zc[1]; d.n_sig = L.word; }
    else for (int i = 0; i < 14; i++) K[K_PUB + i] = pub[i];
    unsigned lg = L.log_N;
    for (uint32_t l = 0; l < L.n_layers; l++) { K[K_WL + l] = root_of_unity(lg); lg -= L.log_f; }
    for (uint32_t i = 0; i < I.a.npub; i++) d.pub[i] = pub[i];
    d.hash = L.opt[3]; d.grinding = L.opt[2]; d.log_rem = ilog2(L.opt[6]);
    for (uint32_t l = 0; l < VMAX_LAYERS; l++) d.npos[l] = l < L.n_layers ? L.npos[l] : 0;
}

template <int M> Lagrange<M> lagrange_weights(uint32_t K) {
    // weights of t -> (the adjoined root) for samples at t = 0..K-1: lag_j = prod_{q != j} (root - q) / (j - q)
    using namespace host;
    Lagrange<M> L{};
    if (M == 1) { L.w[0][0] = ONE; return L; }
    for (uint32_t j = 0; j < K; j++) {
        EX num = ex_one();
        uint64_t den = ONE;
        for (uint32_t q = 0; q < K; q++) {
            if (q == j) continue;
            EX r = ex_zero();
            r.c[0] = sub(0, from_u64(q));
            r.c[1] = ONE;
            num = ex_mul(num, r, M);
            den = mul(den, j > q ? from_u64(j - q) : sub(0, from_u64(q - j)));
        }
        const EX w = ex_scale(num, inv(den));
        for (int c = 0; c < M; c++) L.w[j][c] = w.c[c];
    }
    return L;
}

// the cached coefficients of the proof's periodic columns (header_ok has passed); off = their word offset in the cache
int ensure_pcoef(cstark_ctx *c, VerifyArena *a, const Layout &L, uint64_t &off) {
    constexpr size_t TX_WORDS = 48 * 1024, MK_WORDS = 33 * 512, RS_WORDS = 29 * 8, SC_WORDS = 36 * 512;
    off = 0;
    if (L.air == CSTARK_AIR_RANGE) return CSTARK_OK;
    const bool by_depth = L.air == CSTARK_AIR_STATE_TRANSITION || L.air == CSTARK_AIR_MERKLE_UPDATE;
    const uint32_t dslot = by_depth ? ilog2(L.word + 1) - 1 : 0;
    const uint32_t slot = L.air == CSTARK_AIR_STATE_TRANSITION ? dslot : L.air == CSTARK_AIR_MERKLE_UPDATE ? 6 + dslot : L.air == CSTARK_AIR_RESCUE_CHAIN ? 12 : 13;
    off = L.air == CSTARK_AIR_STATE_TRANSITION ? dslot * TX_WORDS : L.air == CSTARK_AIR_MERKLE_UPDATE ? 6 * TX_WORDS + dslot * MK_WORDS
          : 6 * (TX_WORDS + MK_WORDS) + (L.air == CSTARK_AIR_SCHNORR ? RS_WORDS : 0);
    if (!a->d_pcoef) HIP_TRY(hipMalloc(&a->d_pcoef, (6 * (TX_WORDS + MK_WORDS) + RS_WORDS + SC_WORDS) * 8));
    if (a->pcoef_ready[slot]) return CSTARK_OK;
    std::vector<uint64_t> cols;
    uint32_t ncols, log_cycle;
    if (L.air == CSTARK_AIR_STATE_TRANSITION) {
        if (!host::tx_periodic_columns(L.word, cols)) return fail(CSTARK_ERR_INVALID_ARG, "unsupported Merkle depth");
        ncols = 48; log_cycle = 10;
    } else if (L.air == CSTARK_AIR_MERKLE_UPDATE) {
        if (!host::merkle_periodic_columns(L.word, cols)) return fail(CSTARK_ERR_INVALID_ARG, "unsupported Merkle depth");
        ncols = 33; log_cycle = 9;
    } else if (L.air == CSTARK_AIR_SCHNORR) {
        host::schnorr_mask_columns(cols);
        ncols = 36; log_cycle = 9;
    } else {
        host::rescue_chain_periodic_columns(cols);
        ncols = 29; log_cycle = 3;
    }
    for (uint32_t col = 0; col < ncols; col++) host::intt_small(cols.data() + ((size_t)col << log_cycle), log_cycle);
    HIP_TRY(hipMemcpyAsync(a->d_pcoef + off, cols.data(), cols.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    a->pcoef_ready[slot] = true;
    return CSTARK_OK;
}

// the two launches that leave the statements' 31 values at z in the device region (m = extension degree, tiles = those of the largest statement)
int launch_schnorr_public(uint32_t m, uint32_t tiles, uint32_t G, const uint8_t *buf, const VDesc *desc, const uint32_t *gp, const uint64_t *tb, uint64_t *sp,
                          hipStream_t s) {
    const dim3 grid(tiles, G), block(64 * SCH_TILE);
    if (m == 1) {
        hipLaunchKernelGGL(k_vfy_schnorr_public<1>, grid, block, 0, s, buf, desc, gp, tb, sp);
        hipLaunchKernelGGL(k_vfy_schnorr_public_sum<1>, dim3(G), dim3(64), 0, s, desc, gp, tb, sp);
    } else if (m == 2) {
        hipLaunchKernelGGL(k_vfy_schnorr_public<2>, grid, block, 0, s, buf, desc, gp, tb, sp);
        hipLaunchKernelGGL(k_vfy_schnorr_public_sum<2>, dim3(G), dim3(64), 0, s, desc, gp, tb, sp);
    } else {
        hipLaunchKernelGGL(k_vfy_schnorr_public<3>, grid, block, 0, s, buf, desc, gp, tb, sp);
        hipLaunchKernelGGL(k_vfy_schnorr_public_sum<3>, dim3(G), dim3(64), 0, s, desc, gp, tb, sp);
    }
    HIP_TRY(hipGetLastError());
    return CSTARK_OK;
}

template <class T> T *carve(uint8_t *base, size_t &off, size_t count) {
    off = (off + 15) & ~(size_t)15;
    T *p = reinterpret_cast<T *>(base + off);
    off += count * sizeof(T);
    return p;
}

// Verifies the staged proofs of one chunk; verdicts[i] for staged[i].
int run_chunk(cstark_ctx *c, VerifyArena *a, std::vector<Staged> &st, int32_t *out, double host_ms, const Convert *cv) {
    const hipStream_t s = c->stream;
    const uint32_t P = (uint32_t)st.size();
    // ---- staging block: proofs (a SchnorrAir proof is followed by its statement) | descriptors | openings | group lists; the transcript
    // blocks and the statements' values at z live on the device only
    size_t off = 0, t_words = 0, sp_words = 0;
    std::vector<size_t> pofs(P), tofs(P);
    size_t n_open = 0, n_multi = 0, n_slots = 0; // opened rows of the plain proofs, trees of the compact ones
    size_t n_expand = 0, n_select = 0, out_bytes = 0; // convert calls: trees to expand (among n_multi), trees to select from, the output block
    for (uint32_t i = 0; i < P; i++) {
        const Layout &L = st[i].L;
        off = (off + 15) & ~(size_t)15; pofs[i] = off; off += L.rem + 8 * (size_t)L.R * L.m;
        if (st[i].stm) {
            off = (off + 7) & ~(size_t)7; st[i].d.stmt = off; off += SCH_STATEMENT_BYTES * (size_t)L.word;
            st[i].d.sp = sp_words; sp_words += (size_t)SCH_PUBLIC * L.m * (schnorr_tiles(L.word) + 1);
        }
        tofs[i] = t_words; t_words += (toff(st[i].d.a, L.m, L.n_layers, L.nq).words + 1) & ~(size_t)1;
        uint32_t no = 2 * L.nq;
        for (uint32_t l = 0; l < L.n_layers; l++) no += L.npos[l];
        if (L.form == CSTARK_FORM_COMPACT) { no = 2 + L.n_layers; n_multi += no; }
        else n_open += no;
        st[i].d.n_open = no;
        st[i].d.slot0 = (uint32_t)n_slots;
        n_slots += 1 + no + L.nq + L.m;
        if (cv && L.form != cv->form) { // the output block holds every tree's paths: the new sections, or room for the nodes selected from them
            if (L.form == CSTARK_FORM_COMPACT) n_expand += 2 + L.n_layers;
            else { st[i].count_at = (uint32_t)n_select; n_select += 2 + L.n_layers; }
            for (uint32_t t = 0; t < 2 + L.n_layers; t++) {
                const uint32_t np = t < 2 ? L.nq : L.npos[t - 2];
                st[i].out_at[t] = out_bytes;
                out_bytes += 32 * (size_t)np * (t < 2 ? L.log_N : layer_log_rows(L, t - 2));
            }
        }
    }
    const size_t desc_off = (off + 15) & ~(size_t)15;
    const size_t open_off = (desc_off + P * sizeof(VDesc) + 15) & ~(size_t)15;
    const size_t multi_off = (open_off + n_open * sizeof(VOpen) + 15) & ~(size_t)15; // (no compact proof: empty, the block is as before)
    const size_t grp_off = (multi_off + n_multi * sizeof(VMulti) + 15) & ~(size_t)15;
    // a convert call: behind the group lists, the output offset of every tree that is expanded (in the order of their records) and the
    // trees that are selected from.  A verify call stages what it staged.
    const size_t xat_off = (grp_off + (size_t)P * 4 + 15) & ~(size_t)15;
    const size_t sel_off = (xat_off + n_expand * sizeof(uint64_t) + 15) & ~(size_t)15;
    const size_t copy_bytes = cv ? sel_off + n_select * sizeof(VSelect) : grp_off + (size_t)P * 4;
    const size_t total = copy_bytes + 16;
    if (total > a->stage_bytes) {
        HIP_TRY(hipStreamSynchronize(s));
        if (a->h_stage) { HIP_TRY(hipHostFree(a->h_stage)); a->h_stage = nullptr; }
        if (a->d_stage) { HIP_TRY(hipFree(a->d_stage)); a->d_stage = nullptr; }
        a->stage_bytes = 0;
        HIP_TRY(hipHostMalloc(&a->h_stage, total, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&a->d_stage, total));
        a->stage_bytes = total;
    }
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *H = a->h_stage;
    VDesc *hd = reinterpret_cast<VDesc *>(H + desc_off);
    VOpen *ho = reinterpret_cast<VOpen *>(H + open_off);
    VMulti *hm = reinterpret_cast<VMulti *>(H + multi_off);
    uint32_t *hg = reinterpret_cast<uint32_t *>(H + grp_off); // [P]: the proofs of each (AIR, extension degree), group after group
    // samples per frame: a constraint of degree <= D in the frame has degree <= D (m - 1) along t; any K above that is exact
    Group grp[5 * 3];
    for (uint32_t i = 0; i < P; i++) {
        Group &g = grp[st[i].L.air * 3 + st[i].L.m - 1];
        g.count++;
        g.K = st[i].L.m == 1 ? 1 : st[i].D * (st[i].L.m - 1) + 4;
        if (st[i].stm) g.tiles = std::max(g.tiles, schnorr_tiles(st[i].L.word));
    }
    for (uint32_t g = 0, o = 0; g < 15; g++) { grp[g].start = o; o += grp[g].count; grp[g].frames = grp[g].count * grp[g].K; grp[g].count = 0; }
    std::vector<VOpen> opens;
    opens.reserve(n_open);
    std::vector<VMulti> multis;
    multis.reserve(n_multi);
    std::vector<std::pair<VMulti, uint64_t>> expands; // convert calls: the trees of the proofs that are expanded, and where their paths go
    std::vector<VSelect> selects;                     // ... the trees of the proofs that are compacted
    expands.reserve(n_expand);
    selects.reserve(n_select);
    for (uint32_t i = 0; i < P; i++) {
        Staged &S = st[i];
        const Layout &L = S.L;
        memcpy(H + pofs[i], S.bytes, L.rem + 8 * (size_t)L.R * L.m);
        VDesc &d = S.d;
        if (S.stm) {
            // the statement in the order of the channel seed: messages, R.x (canonical words there), the s halves; the seed message is
            // up to 155 KB and SHA3 is sequential, so its digest is taken here, by the prover's own statement of it
            const size_t ns = L.word;
            uint8_t *sm = H + d.stmt;
            memcpy(sm, S.stm->messages, 8 * 28 * ns); memcpy(sm + 8 * 28 * ns, S.stm->sig_rx, 8 * 6 * ns); memcpy(sm + 8 * 34 * ns, S.stm->sig_s, 32 * ns);
            cstark_options o;
            memcpy(&o.num_queries, L.opt, sizeof L.opt);
            const std::vector<uint8_t> seed = transcript::channel_seed(L.width, L.log_n, o, L.log_b, ilog2(L.opt[6]), reinterpret_cast<const uint64_t *>(sm),
                                                                       34 * ns, sm + 8 * 34 * ns, 32 * ns);
            uint8_t dg[32];
            digest(L.opt[3], seed.data(), seed.size(), dg);
            memcpy(d.seed, dg, 32);
        }
        d.base = pofs[i]; d.tb = tofs[i];
        d.ood = (uint32_t)L.ood; d.trows = (uint32_t)L.trows; d.tpaths = (uint32_t)L.tpaths; d.crows = (uint32_t)L.crows;
        d.cpaths = (uint32_t)L.cpaths; d.rem = (uint32_t)L.rem;
        for (uint32_t l = 0; l < VMAX_LAYERS; l++) d.lrows[l] = (uint32_t)L.lrows[l];
        d.log_n = L.log_n; d.log_N = L.log_N; d.nq = L.nq; d.log_f = L.log_f; d.n_layers = L.n_layers; d.m = L.m; d.R = L.R; d.log_b = L.log_b;
        Group &g = grp[L.air * 3 + L.m - 1];
        hg[g.start + g.count++] = i;
        hd[i] = d;
        const uint32_t TW = d.a.w, TCE = d.a.ce;
        const uint32_t hash = L.opt[3];
        uint32_t sl = d.slot0 + 1;
        const bool changes = cv && L.form != cv->form;
        if (L.form == CSTARK_FORM_COMPACT) { // one entry per tree, in the verdict order: trace, composition, the layers
            uint32_t t = 0;
            auto tree = [&](const VMulti &m) { // a proof that is expanded: the same record, for k_vfy_multi_expand
                if (changes) expands.emplace_back(m, (uint64_t)S.out_at[t]);
                else multis.push_back(m);
                t++;
            };
            tree(VMulti{i, (uint32_t)L.trows, (uint32_t)L.tpaths, L.nodes[0], 52u, TW, L.log_N, VNO_LAYER, L.nq, RK_OPENING0, sl++, hash});
            tree(VMulti{i, (uint32_t)L.crows, (uint32_t)L.cpaths, L.nodes[1], 84u, TCE * L.m, L.log_N, VNO_LAYER, L.nq, RK_OPENING0 + 1, sl++, hash});
            for (uint32_t l = 0; l < L.n_layers; l++)
                tree(VMulti{i, (uint32_t)L.lrows[l], (uint32_t)L.lpaths[l], L.nodes[2 + l], (uint32_t)(120 + 32 * l), L.f * L.m,
                            layer_log_rows(L, l), l, L.npos[l], RK_LAYER0 + 3 * l + 1, sl++, hash});
            continue;
        }
        if (changes) { // a plain proof that is compacted: its opening records below as ever, and one selection per tree
            selects.push_back(VSelect{i, (uint32_t)L.tpaths, L.log_N, VNO_LAYER, L.nq, S.count_at, (uint64_t)S.out_at[0]});
            selects.push_back(VSelect{i, (uint32_t)L.cpaths, L.log_N, VNO_LAYER, L.nq, S.count_at + 1, (uint64_t)S.out_at[1]});
            for (uint32_t l = 0; l < L.n_layers; l++)
                selects.push_back(VSelect{i, (uint32_t)L.lpaths[l], layer_log_rows(L, l), l, L.npos[l], S.count_at + 2 + l, (uint64_t)S.out_at[2 + l]});
        }
        for (uint32_t q = 0; q < L.nq; q++) {
            opens.push_back(VOpen{i, (uint32_t)(L.trows + 8 * (size_t)q * TW), (uint32_t)(L.tpaths + 32 * (size_t)q * L.log_N), 52u, TW, L.log_N,
                                  VNO_LAYER, q, RK_OPENING0 + 2 * q, sl++, hash});
            opens.push_back(VOpen{i, (uint32_t)(L.crows + 8 * (size_t)q * TCE * L.m), (uint32_t)(L.cpaths + 32 * (size_t)q * L.log_N), 84u,
                                  TCE * L.m, L.log_N, VNO_LAYER, q, RK_OPENING0 + 2 * q + 1, sl++, hash});
        }
        unsigned lg = L.log_N;
        // every layer's rows: from the first layer whose count differs (LAYER_COUNT, found by the replay) there are no positions to
        // check the paths against, but their words must still be canonical -- those lanes report MALFORMED only
        for (uint32_t l = 0; l < L.n_layers; l++) {
            const uint32_t depth = lg - L.log_f;
            for (uint32_t t = 0; t < L.npos[l]; t++)
                opens.push_back(VOpen{i, (uint32_t)(L.lrows[l] + 8 * (size_t)t * L.f * L.m), (uint32_t)(L.lpaths[l] + 32 * (size_t)t * depth),
                                      (uint32_t)(120 + 32 * l), L.f * L.m, depth, l, t, RK_LAYER0 + 3 * l + 1, sl++, hash});
            lg = depth;
        }
    }
    // the lanes of a wave walk paths of one hash and one length: no divergence between trace paths of 23 levels and layer paths of 7
    std::stable_sort(opens.begin(), opens.end(), [](const VOpen &x, const VOpen &y) {
        return x.hash != y.hash ? x.hash < y.hash : x.words != y.words ? x.words < y.words : x.depth < y.depth;
    });
    memcpy(ho, opens.data(), opens.size() * sizeof(VOpen));
    // the trees of one hash side by side: one launch of k_vfy_multi_open per hash present
    const size_t n_multi_b3 = std::stable_partition(multis.begin(), multis.end(), [](const VMulti &x) { return x.hash == 0; }) - multis.begin();
    if (n_multi) memcpy(hm, multis.data(), multis.size() * sizeof(VMulti));
    // behind them the trees that are expanded, again one hash after the other, each with its place in the output block
    const size_t n_open_multi = multis.size();
    const size_t n_expand_b3 = std::stable_partition(expands.begin(), expands.end(), [](const std::pair<VMulti, uint64_t> &x) { return x.first.hash == 0; }) - expands.begin();
    for (size_t k = 0; k < n_expand; k++) {
        hm[n_open_multi + k] = expands[k].first;
        reinterpret_cast<uint64_t *>(H + xat_off)[k] = expands[k].second;
    }
    if (n_select) memcpy(H + sel_off, selects.data(), n_select * sizeof(VSelect));
    const auto t1 = std::chrono::steady_clock::now();
    host_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();

    // ---- device scratch: transcript blocks | slots | verdicts | per group: frames cur, next, per, values | bad flags
    size_t need = 8 * t_words + 16;
    need += 8 * sp_words + 16;
    need += 4 * n_slots + 16;
    need += 4 * (size_t)P + 16;
    for (uint32_t g = 0; g < 15; g++)
        if (grp[g].count) {
            const VAir &A = air_info(g / 3).a;
            need += 8 * (size_t)grp[g].frames * (2 * A.w + A.nper + A.naux + A.nc) + 4 * (size_t)grp[g].count + 5 * 16;
        }
    // a convert call: the output block behind them -- the node counts of the selected trees, then every changing tree's region
    const size_t counts_bytes = (4 * n_select + 31) & ~(size_t)31, block_bytes = counts_bytes + out_bytes;
    if (block_bytes) need += block_bytes + 16;
    if (need > a->scratch_bytes) {
        HIP_TRY(hipStreamSynchronize(s));
        if (a->d_scratch) { HIP_TRY(hipFree(a->d_scratch)); a->d_scratch = nullptr; }
        a->scratch_bytes = 0;
        HIP_TRY(hipMalloc(&a->d_scratch, need));
        a->scratch_bytes = need;
    }
    if (P > a->verdict_cap) {
        if (a->h_verdicts) { HIP_TRY(hipHostFree(a->h_verdicts)); a->h_verdicts = nullptr; }
        a->verdict_cap = 0;
        HIP_TRY(hipHostMalloc(&a->h_verdicts, 4 * (size_t)P, hipHostMallocDefault));
        a->verdict_cap = P;
    }
    uint8_t *D = (uint8_t *)a->d_scratch;
    size_t so = 0;
    uint64_t *d_tb = carve<uint64_t>(D, so, t_words);
    uint64_t *d_sp = carve<uint64_t>(D, so, sp_words);
    uint32_t *d_slots = carve<uint32_t>(D, so, n_slots);
    int32_t *d_verd = carve<int32_t>(D, so, P);
    for (uint32_t g = 0; g < 15; g++) {
        if (!grp[g].count) continue;
        const VAir &A = air_info(g / 3).a;
        grp[g].cur = carve<fp>(D, so, (size_t)grp[g].frames * A.w);
        grp[g].nxt = carve<fp>(D, so, (size_t)grp[g].frames * A.w);
        grp[g].per = carve<fp>(D, so, (size_t)grp[g].frames * (A.nper + A.naux));
        grp[g].val = carve<fp>(D, so, (size_t)grp[g].frames * A.nc);
        grp[g].bad = carve<uint32_t>(D, so, grp[g].count);
    }
    uint8_t *d_block = block_bytes ? carve<uint8_t>(D, so, block_bytes) : nullptr;
    if (block_bytes > a->out_bytes) {
        if (a->h_out) { HIP_TRY(hipHostFree(a->h_out)); a->h_out = nullptr; }
        a->out_bytes = 0;
        HIP_TRY(hipHostMalloc(&a->h_out, block_bytes, hipHostMallocDefault));
        a->out_bytes = block_bytes;
    }
    const uint8_t *dbuf = a->d_stage;
    const VDesc *d_desc = reinterpret_cast<const VDesc *>(dbuf + desc_off);
    const VOpen *d_open = reinterpret_cast<const VOpen *>(dbuf + open_off);
    const VMulti *d_multi = reinterpret_cast<const VMulti *>(dbuf + multi_off);
    const uint32_t *d_grp = reinterpret_cast<const uint32_t *>(dbuf + grp_off);

    for (int e = 0; e < VFY_EVENTS; e++)
        if (!a->ev[e]) HIP_TRY(hipEventCreate(&a->ev[e]));
    HIP_TRY(hipEventRecord(a->ev[0], s));
    HIP_TRY(hipMemcpyAsync(a->d_stage, H, copy_bytes, hipMemcpyHostToDevice, s));
    a->h2d_bytes += copy_bytes;
    HIP_TRY(hipEventRecord(a->ev[1], s));
    hipLaunchKernelGGL(k_vfy_transcript, dim3(P), dim3(VT), 0, s, dbuf, d_desc, d_tb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(a->ev[2], s));
    for (uint32_t g = 0; g < 15; g++) {
        const Group &Gr = grp[g];
        const uint32_t G = Gr.count, mi = g % 3, air = g / 3;
        if (!G) continue;
        const uint32_t F = Gr.frames, K = Gr.K;
        const uint32_t *gp = d_grp + Gr.start;
        if (air == CSTARK_AIR_SCHNORR) RC_TRY(launch_schnorr_public(mi + 1, Gr.tiles, G, dbuf, d_desc, gp, d_tb, d_sp, s));
        if (mi == 0) {
            hipLaunchKernelGGL(k_vfy_ood_frames<1>, dim3(G), dim3(128), 0, s, dbuf, d_desc, gp, d_tb, a->d_pcoef, d_sp, K, F, Gr.cur, Gr.nxt, Gr.per, Gr.bad);
        } else if (mi == 1) {
            hipLaunchKernelGGL(k_vfy_ood_frames<2>, dim3(G), dim3(128), 0, s, dbuf, d_desc, gp, d_tb, a->d_pcoef, d_sp, K, F, Gr.cur, Gr.nxt, Gr.per, Gr.bad);
        } else {
            hipLaunchKernelGGL(k_vfy_ood_frames<3>, dim3(G), dim3(128), 0, s, dbuf, d_desc, gp, d_tb, a->d_pcoef, d_sp, K, F, Gr.cur, Gr.nxt, Gr.per, Gr.bad);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_eval_frames_air((int)air, Gr.cur, Gr.nxt, Gr.per, Gr.val, F, s));
        const dim3 cg((G + 63) / 64);
        const VGroups &vg = air_info(air).groups;
        const VAsserts &va = air_info(air).asserts;
        if (mi == 0) hipLaunchKernelGGL(k_vfy_ood_check<1>, cg, dim3(64), 0, s, dbuf, d_desc, gp, G, K, F, Gr.val, Gr.bad, lagrange_weights<1>(K), vg, va, d_sp, d_tb, d_slots);
        else if (mi == 1) hipLaunchKernelGGL(k_vfy_ood_check<2>, cg, dim3(64), 0, s, dbuf, d_desc, gp, G, K, F, Gr.val, Gr.bad, lagrange_weights<2>(K), vg, va, d_sp, d_tb, d_slots);
        else hipLaunchKernelGGL(k_vfy_ood_check<3>, cg, dim3(64), 0, s, dbuf, d_desc, gp, G, K, F, Gr.val, Gr.bad, lagrange_weights<3>(K), vg, va, d_sp, d_tb, d_slots);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(a->ev[3], s));
    if (n_open) {
        hipLaunchKernelGGL(k_vfy_openings, dim3((unsigned)((n_open + 127) / 128)), dim3(128), 0, s, dbuf, d_desc, d_open, (uint32_t)n_open, d_tb, d_slots);
        HIP_TRY(hipGetLastError());
    }
    if (n_multi_b3) {
        hipLaunchKernelGGL(k_vfy_multi_open<0>, dim3((unsigned)n_multi_b3), dim3(128), 0, s, dbuf, d_desc, d_multi, d_tb, d_slots);
        HIP_TRY(hipGetLastError());
    }
    if (n_open_multi > n_multi_b3) {
        hipLaunchKernelGGL(k_vfy_multi_open<1>, dim3((unsigned)(n_open_multi - n_multi_b3)), dim3(128), 0, s, dbuf, d_desc, d_multi + n_multi_b3, d_tb, d_slots);
        HIP_TRY(hipGetLastError());
    }
    // a convert call: the trees that are expanded fold in k_vfy_multi_expand instead, the plain proofs that are compacted are selected from
    const uint64_t *d_xat = reinterpret_cast<const uint64_t *>(dbuf + xat_off);
    uint8_t *d_out = d_block + counts_bytes;
    if (n_expand_b3) {
        hipLaunchKernelGGL(k_vfy_multi_expand<0>, dim3((unsigned)n_expand_b3), dim3(128), 0, s, dbuf, d_desc, d_multi + n_open_multi, d_tb, d_slots, d_xat, d_out);
        HIP_TRY(hipGetLastError());
    }
    if (n_expand > n_expand_b3) {
        hipLaunchKernelGGL(k_vfy_multi_expand<1>, dim3((unsigned)(n_expand - n_expand_b3)), dim3(128), 0, s, dbuf, d_desc, d_multi + n_open_multi + n_expand_b3,
                           d_tb, d_slots, d_xat + n_expand_b3, d_out);
        HIP_TRY(hipGetLastError());
    }
    if (n_select) {
        hipLaunchKernelGGL(k_vfy_multi_select, dim3((unsigned)n_select), dim3(128), 0, s, dbuf, d_desc, reinterpret_cast<const VSelect *>(dbuf + sel_off), d_tb,
                           reinterpret_cast<uint32_t *>(d_block), d_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(a->ev[4], s));
    for (uint32_t g = 0; g < 15; g++) {
        const uint32_t G = grp[g].count, mi = g % 3;
        if (!G) continue;
        const dim3 grid(1, G); // num_queries <= 128: one workgroup per proof
        if (mi == 0) hipLaunchKernelGGL(k_vfy_fri<1>, grid, dim3(128), 0, s, dbuf, d_desc, d_grp + grp[g].start, d_tb, d_slots);
        else if (mi == 1) hipLaunchKernelGGL(k_vfy_fri<2>, grid, dim3(128), 0, s, dbuf, d_desc, d_grp + grp[g].start, d_tb, d_slots);
        else hipLaunchKernelGGL(k_vfy_fri<3>, grid, dim3(128), 0, s, dbuf, d_desc, d_grp + grp[g].start, d_tb, d_slots);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(a->ev[5], s));
    hipLaunchKernelGGL(k_vfy_remainder, dim3(3, P), dim3(256), 0, s, dbuf, d_desc, d_tb, d_slots);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vfy_reduce, dim3(P), dim3(256), 0, s, d_desc, d_tb, d_slots, d_verd);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a->h_verdicts, d_verd, 4 * (size_t)P, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(a->ev[6], s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < P; i++) out[st[i].index] = a->h_verdicts[i];
    a->ms[0] += (float)host_ms;
    for (int e = 1; e < VFY_EVENTS; e++) {
        float t;
        HIP_TRY(hipEventElapsedTime(&t, a->ev[e - 1], a->ev[e]));
        a->ms[e] += t;
    }
    if (!cv) return CSTARK_OK;
    // ---- a convert call: the accepted proofs in the target form.  One copy back of the part of the output block that accepted proofs
    // own (and the selected trees' counts), after the verdicts: nothing is copied for a chunk without an accepted proof that changes.
    size_t lo = out_bytes, hi = 0;
    bool selected = false;
    for (uint32_t i = 0; i < P; i++) {
        const Layout &L = st[i].L;
        if (a->h_verdicts[i] != CSTARK_PROOF_OK || L.form == cv->form) continue;
        const TreeSection last = tree_section(L, 1 + L.n_layers);
        lo = std::min(lo, st[i].out_at[0]);
        hi = std::max(hi, st[i].out_at[1 + L.n_layers] + 32 * (size_t)last.count * last.depth);
        selected |= L.form == CSTARK_FORM_PLAIN;
    }
    const auto c0 = std::chrono::steady_clock::now();
    if (selected) HIP_TRY(hipMemcpyAsync(a->h_out, d_block, 4 * n_select, hipMemcpyDeviceToHost, s));
    if (hi > lo) HIP_TRY(hipMemcpyAsync(a->h_out + counts_bytes + lo, d_out + lo, hi - lo, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const auto c1 = std::chrono::steady_clock::now();
    a->ms[VFY_EVENTS - 1] += (float)std::chrono::duration<double, std::milli>(c1 - c0).count();
    const uint32_t *counts = reinterpret_cast<const uint32_t *>(a->h_out);
    for (uint32_t i = 0; i < P; i++) {
        const Layout &L = st[i].L;
        if (a->h_verdicts[i] != CSTARK_PROOF_OK) continue;
        PathSections ps{};
        for (uint32_t t = 0; L.form != cv->form && t < 2 + L.n_layers; t++) {
            ps.data[t] = a->h_out + counts_bytes + st[i].out_at[t];
            if (L.form == CSTARK_FORM_PLAIN) ps.nodes[t] = counts[st[i].count_at + t];
        }
        const uint32_t at = st[i].index;
        if (convert_proof(st[i].bytes, L, cv->form, ps, cv->out[at], cv->capacities[at], &cv->out_lens[at]) != CSTARK_OK)
            return fail(CSTARK_ERR_INVALID_ARG, "convert: a proof does not fit the capacity that was checked");
    }
    a->ms[0] += (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c1).count();
    return CSTARK_OK;
}

} // namespace
} // namespace cs

using namespace cs;

extern "C" {

int cstark_proof_inspect(const uint8_t *proof, size_t len, cstark_proof_info *info, int32_t *verdict) {
    if (!proof || !info || !verdict) return fail(CSTARK_ERR_INVALID_ARG, "cstark_proof_inspect: null argument");
    Layout L;
    *verdict = parse_layout(proof, len, L);
    memset(info, 0, sizeof *info);
    // the header words as read (all zero unless the magic matched)
    info->air = L.air; info->trace_width = L.width; info->log_n = L.log_n; info->header_word = L.word;
    memcpy(&info->options, L.opt, sizeof L.opt);
    return CSTARK_OK;
}

int cstark_proof_form(const uint8_t *proof, size_t len, uint32_t *form) {
    if (!proof || !form) return fail(CSTARK_ERR_INVALID_ARG, "cstark_proof_form: null argument");
    const int f = proof_form_of(proof, len);
    if (f < 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_proof_form: neither a plain nor a compact proof");
    *form = (uint32_t)f;
    return CSTARK_OK;
}

// All verify calls.  airs: the AIR the caller states for each proof (null: all TransactionAir); the 14 public words of proof i are
// pub_lo[i * stride .. +7) | pub_hi[i * stride .. +7).  stm (cstark_schnorr_verify; then airs and the public words are null): every proof is
// stated to be SchnorrAir's, with statement stm[i].  cv (the convert calls; null: a verify call): every accepted proof is also written to
// the caller's buffer in cv->form; the verdicts are those of the verify call.
static int verify_batch(const char *who, cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *airs,
                        const uint64_t *pub_lo, const uint64_t *pub_hi, size_t stride, const cstark_schnorr_statement *stm,
                        const cstark_options *expected, int32_t *verdicts, const Convert *cv = nullptr) {
    if (!c) return fail(CSTARK_ERR_INVALID_ARG, "%s: null context", who);
    if (cv && cv->form != CSTARK_FORM_PLAIN && cv->form != CSTARK_FORM_COMPACT)
        return fail(CSTARK_ERR_INVALID_ARG, "%s: form must be CSTARK_FORM_PLAIN or CSTARK_FORM_COMPACT", who);
    if (count == 0) return CSTARK_OK;
    if (!proofs || !proof_lens || (!stm && (!pub_lo || !pub_hi)) || !verdicts) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (cv && (!cv->out || !cv->capacities || !cv->out_lens)) return fail(CSTARK_ERR_INVALID_ARG, "%s: null output argument", who);
    for (uint32_t i = 0; stm && i < count; i++) {
        const cstark_schnorr_statement &S = stm[i];
        if (!S.messages || !S.sig_rx || !S.sig_s) return fail(CSTARK_ERR_INVALID_ARG, "%s: null statement array", who);
        if (S.n_sig == 0) return fail(CSTARK_ERR_INVALID_ARG, "%s: a statement without signatures", who);
        for (size_t k = 0; k < 28 * (size_t)S.n_sig; k++)
            if (S.messages[k] >= host::P) return fail(CSTARK_ERR_INVALID_ARG, "%s: a message word is not a field element", who);
        for (size_t k = 0; k < 6 * (size_t)S.n_sig; k++)
            if (S.sig_rx[k] >= host::P) return fail(CSTARK_ERR_INVALID_ARG, "%s: an R.x word is not a field element", who);
        if (!proofs[i] && proof_lens[i]) return fail(CSTARK_ERR_INVALID_ARG, "%s: null proof", who);
    }
    for (uint32_t i = 0; !stm && i < count; i++) {
        const int32_t air = airs ? airs[i] : (int32_t)CSTARK_AIR_STATE_TRANSITION;
        if (air < 0 || air > 4) return fail(CSTARK_ERR_INVALID_ARG, "%s: unknown AIR id", who);
        const uint32_t used = air == CSTARK_AIR_SCHNORR ? 0 : air == CSTARK_AIR_RANGE ? 1 : 14; // SchnorrAir: never verified, nothing read
        for (uint32_t k = 0; k < used; k++)
            if ((k < 7 ? pub_lo[i * stride + k] : pub_hi[i * stride + k - 7]) >= host::P)
                return fail(CSTARK_ERR_INVALID_ARG, "%s: a public input word is not a field element", who);
        if (!proofs[i] && proof_lens[i]) return fail(CSTARK_ERR_INVALID_ARG, "%s: null proof", who);
    }
    // every capacity before anything is launched, for every proof whose layout parses: no output is written by a call that is refused
    for (uint32_t i = 0; cv && i < count; i++) {
        Layout L;
        if (!proofs[i] || parse_layout(proofs[i], proof_lens[i], L) != CSTARK_PROOF_OK) continue;
        const size_t bound = convert_bound(L, cv->form);
        if (!cv->out[i] || cv->capacities[i] < bound) {
            char msg[160];
            snprintf(msg, sizeof msg, "%s: the buffer of proof %u holds %zu bytes, cstark_proof_convert_bound asks for %zu", who, i,
                     cv->out[i] ? cv->capacities[i] : (size_t)0, bound);
            return fail(CSTARK_ERR_INVALID_ARG, "%s", msg);
        }
    }
    for (uint32_t i = 0; cv && i < count; i++) cv->out_lens[i] = 0;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->verify) c->verify = new VerifyArena();
    VerifyArena *a = c->verify;
    for (float &m : a->ms) m = 0;
    a->h2d_bytes = 0;
    a->timed = false;
    std::vector<Staged> st;
    size_t chunk_bytes = 0;
    double host_ms = 0;
    auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < count; i++) {
        const uint8_t *b = proofs[i];
        const uint32_t air = stm ? (uint32_t)CSTARK_AIR_SCHNORR : airs ? (uint32_t)airs[i] : (uint32_t)CSTARK_AIR_STATE_TRANSITION;
        Staged S;
        S.index = i;
        S.bytes = b;
        int v = b ? parse_layout(b, proof_lens[i], S.L) : CSTARK_PROOF_MALFORMED;
        // a proof of another AIR than the caller states, or of SchnorrAir through a call that carries no statement for it: no kernel reads
        // it, so its elements are scanned here (a word >= p is MALFORMED before UNSUPPORTED)
        const AirInfo &I = air_info(air);
        if (v == CSTARK_PROOF_OK && (S.L.air != air || !I.ok || (air == CSTARK_AIR_SCHNORR && !stm)))
            v = elements_canonical(b, S.L) ? CSTARK_PROOF_UNSUPPORTED : CSTARK_PROOF_MALFORMED;
        if (v == CSTARK_PROOF_OK && !header_ok(S.L)) v = CSTARK_PROOF_MALFORMED;
        if (v == CSTARK_PROOF_OK && expected) {
            const uint32_t *e = &expected->num_queries;
            if (memcmp(e, S.L.opt, sizeof S.L.opt) != 0) v = elements_canonical(b, S.L) ? CSTARK_PROOF_OPTIONS_MISMATCH : CSTARK_PROOF_MALFORMED;
        }
        // a statement of another number of signatures than the header's: its seed and its values at z are not the proof's, decided
        // here so that nothing on the device is sized by the difference (the restated verifier: "proof is for a different number of signatures")
        if (v == CSTARK_PROOF_OK && stm && stm[i].n_sig != S.L.word) v = elements_canonical(b, S.L) ? CSTARK_PROOF_OOD : CSTARK_PROOF_MALFORMED;
        if (v != CSTARK_PROOF_OK) { verdicts[i] = v; continue; }
        if (stm) S.stm = &stm[i];
        memset(&S.d, 0, sizeof S.d);
        S.D = I.D;
        RC_TRY(ensure_pcoef(c, a, S.L, S.d.pcoef));
        uint64_t pub[14] = {};
        for (int k = 0; !stm && k < 7; k++) { pub[k] = pub_lo[i * stride + k]; pub[7 + k] = pub_hi[i * stride + k]; }
        describe(S.L, I, adjustments(a, I, S.L.log_n), pub, S.d);
        const size_t bytes = proof_lens[i] + (stm ? SCH_STATEMENT_BYTES * (size_t)S.L.word : 0) + sizeof(VDesc) +
                             sizeof(VOpen) * (2 + S.L.nq * (size_t)(2 + S.L.n_layers)) + 256;
        if (!st.empty() && chunk_bytes + bytes > VFY_CHUNK_BYTES) {
            host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            RC_TRY(run_chunk(c, a, st, verdicts, host_ms, cv));
            st.clear(); chunk_bytes = 0; host_ms = 0;
            t0 = std::chrono::steady_clock::now();
        }
        st.push_back(std::move(S));
        chunk_bytes += bytes;
    }
    host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!st.empty()) RC_TRY(run_chunk(c, a, st, verdicts, host_ms, cv));
    else a->ms[0] += (float)host_ms;
    a->timed = true;
    return CSTARK_OK;
}

int cstark_tx_verify(cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const uint64_t *initial_roots,
                     const uint64_t *final_roots, const cstark_options *expected, int32_t *verdicts) {
    return verify_batch("cstark_tx_verify", c, count, proofs, proof_lens, nullptr, initial_roots, final_roots, 7, nullptr, expected, verdicts);
}

int cstark_air_verify(cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *airs,
                      const uint64_t *public_inputs, const cstark_options *expected, int32_t *verdicts) {
    if (c && count && (!airs || !public_inputs)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_verify: null argument");
    return verify_batch("cstark_air_verify", c, count, proofs, proof_lens, airs, public_inputs, public_inputs ? public_inputs + 7 : nullptr, 14, nullptr, expected, verdicts);
}

int cstark_schnorr_verify(cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const cstark_schnorr_statement *statements,
                          const cstark_options *expected, int32_t *verdicts) {
    if (c && count && !statements) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_verify: null argument");
    return verify_batch("cstark_schnorr_verify", c, count, proofs, proof_lens, nullptr, nullptr, nullptr, 0, statements, expected, verdicts);
}

int cstark_proof_convert_bound(const uint8_t *proof, size_t len, uint32_t form, size_t *bound) {
    if (!proof || !bound) return fail(CSTARK_ERR_INVALID_ARG, "cstark_proof_convert_bound: null argument");
    if (form != CSTARK_FORM_PLAIN && form != CSTARK_FORM_COMPACT)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_proof_convert_bound: form must be CSTARK_FORM_PLAIN or CSTARK_FORM_COMPACT");
    Layout L;
    if (parse_layout(proof, len, L) != CSTARK_PROOF_OK) return fail(CSTARK_ERR_INVALID_ARG, "cstark_proof_convert_bound: the proof's layout does not parse");
    *bound = convert_bound(L, form);
    return CSTARK_OK;
}

int cstark_tx_convert(cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const uint64_t *initial_roots,
                      const uint64_t *final_roots, const cstark_options *expected, uint32_t form, uint8_t *const *out, const size_t *capacities,
                      size_t *out_lens, int32_t *verdicts) {
    const Convert cv{form, out, capacities, out_lens};
    return verify_batch("cstark_tx_convert", c, count, proofs, proof_lens, nullptr, initial_roots, final_roots, 7, nullptr, expected, verdicts, &cv);
}

int cstark_air_convert(cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *airs,
                       const uint64_t *public_inputs, const cstark_options *expected, uint32_t form, uint8_t *const *out, const size_t *capacities,
                       size_t *out_lens, int32_t *verdicts) {
    if (c && count && (!airs || !public_inputs)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_convert: null argument");
    const Convert cv{form, out, capacities, out_lens};
    return verify_batch("cstark_air_convert", c, count, proofs, proof_lens, airs, public_inputs, public_inputs ? public_inputs + 7 : nullptr, 14, nullptr, expected,
                        verdicts, &cv);
}

int cstark_schnorr_convert(cstark_ctx *c, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const cstark_schnorr_statement *statements,
                           const cstark_options *expected, uint32_t form, uint8_t *const *out, const size_t *capacities, size_t *out_lens,
                           int32_t *verdicts) {
    if (c && count && !statements) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_convert: null argument");
    const Convert cv{form, out, capacities, out_lens};
    return verify_batch("cstark_schnorr_convert", c, count, proofs, proof_lens, nullptr, nullptr, nullptr, 0, statements, expected, verdicts, &cv);
}

// k_vfy_schnorr_public + k_vfy_schnorr_public_sum for one statement and the caller's z, through a descriptor that holds what the two read
int cstark_schnorr_public_at(cstark_ctx *c, uint32_t n_sig, const uint64_t *messages, const uint64_t *sig_rx, const uint64_t *z, uint32_t m, uint64_t *out) {
    using namespace host;
    if (!c || !messages || !sig_rx || !z || !out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: null argument");
    if (m < 1 || m > 3) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: m must be 1, 2 or 3");
    if (n_sig == 0 || (n_sig & (n_sig - 1)) || n_sig > (1u << 12)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: n_sig must be a power of two, at most 4096");
    for (size_t k = 0; k < 28 * (size_t)n_sig; k++) if (messages[k] >= P) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: a message word is not a field element");
    for (size_t k = 0; k < 6 * (size_t)n_sig; k++) if (sig_rx[k] >= P) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: an R.x word is not a field element");
    for (uint32_t q = 0; q < m; q++) if (z[q] >= P) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: z is not a field element");
    const uint32_t log_n = 9 + ilog2(n_sig);
    EX zn = ex_load(z, m);
    for (uint32_t s = 0; s < log_n; s++) zn = ex_mul(zn, zn, m);
    if (zn.c[0] == ONE && zn.c[1] == 0 && zn.c[2] == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_at: z lies on the trace domain");
    HIP_TRY(hipSetDevice(c->device));
    // one block: descriptor | group list | statement | z | partials and values
    const uint32_t tiles = schnorr_tiles(n_sig);
    const size_t o_gp = sizeof(VDesc), o_stmt = (o_gp + 4 + 15) & ~(size_t)15, o_z = o_stmt + 8 * 34 * (size_t)n_sig, o_sp = o_z + 8 * m,
                 total = o_sp + 8 * (size_t)SCH_PUBLIC * m * (tiles + 1);
    std::vector<uint8_t> h(o_sp, 0);
    VDesc *d = reinterpret_cast<VDesc *>(h.data());
    d->a = air_info(CSTARK_AIR_SCHNORR).a;
    d->k[K_WN] = root_of_unity(log_n);
    d->stmt = o_stmt; d->sp = 0; d->tb = 0; d->n_sig = n_sig; d->log_n = log_n; d->m = m;
    memcpy(h.data() + o_stmt, messages, 8 * 28 * (size_t)n_sig);
    memcpy(h.data() + o_stmt + 8 * 28 * (size_t)n_sig, sig_rx, 8 * 6 * (size_t)n_sig);
    memcpy(h.data() + o_z, z, 8 * m);
    uint8_t *dev = nullptr;
    HIP_TRY(hipMalloc(&dev, total));
    int rc = CSTARK_OK;
    hipError_t e = hipMemcpyAsync(dev, h.data(), o_sp, hipMemcpyHostToDevice, c->stream);
    uint64_t *d_sp = reinterpret_cast<uint64_t *>(dev + o_sp);
    if (e == hipSuccess)
        rc = launch_schnorr_public(m, tiles, 1, dev, reinterpret_cast<const VDesc *>(dev), reinterpret_cast<const uint32_t *>(dev + o_gp),
                                   reinterpret_cast<const uint64_t *>(dev + o_z), d_sp, c->stream);
    if (e == hipSuccess && rc == CSTARK_OK)
        e = hipMemcpyAsync(out, d_sp + (size_t)SCH_PUBLIC * m * tiles, 8 * (size_t)SCH_PUBLIC * m, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(dev);
    if (rc != CSTARK_OK) return rc;
    HIP_TRY(e);
    return CSTARK_OK;
}

int cstark_verify_stage_ms(cstark_ctx *c, float *ms) {
    if (!c || !ms) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    if (!c->verify || !c->verify->timed) return fail(CSTARK_ERR_INVALID_ARG, "no verification has run on this context");
    for (int i = 0; i < CSTARK_VERIFY_NUM_STAGES; i++) ms[i] = c->verify->ms[i];
    return CSTARK_OK;
}

int cstark_verify_h2d_bytes(cstark_ctx *c, uint64_t *bytes) {
    if (!c || !bytes) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    if (!c->verify || !c->verify->timed) return fail(CSTARK_ERR_INVALID_ARG, "no verification has run on this context");
    *bytes = c->verify->h2d_bytes;
    return CSTARK_OK;
}

} // extern "C"
