// K2/K3 -- radix-2 NTT over f63 for column-major tables: interpolation (inverse transform) and coset
// low-degree extension.  Engine stage behind `prover.prove(trace)` (/root/reference/src/lib.rs:140;
// winterfell trace.extend [UPSTREAM-RECALL]); the algorithm is the textbook four-step decomposition
// n = R * C, mapped to gfx950 as two kernels per transform:
//
//   k_ntt_cols  one workgroup owns L adjacent matrix columns (all R rows): global accesses are L*8-byte
//               segments at stride C, the R-point sub-transforms run in LDS (DIF, natural in, bit-reversed
//               positions out), the inter-step twiddle w_n^(k1*c) is applied on the way out.
//   k_ntt_rows  one workgroup owns L adjacent rows of the intermediate (each row contiguous in HBM): loads
//               are fully coalesced, the C-point sub-transforms run in LDS, and the store performs the
//               transposition back to natural order (k = k1 + R*k2) in L*8-byte segments.
//
// HBM traffic per transform: read n + write n + read n + write n elements (8 bytes each); twiddle and
// coset-scaling tables (8 MB each at n = 2^20) are shared by all columns and stay in L2 / Infinity Cache.
#include "ntt.h"
#include "fp.cuh"
#include "hostfield.h"
#include "../../include/cstark_conventions.h"
#ifdef CS_NTT_NOMATH // measurement build (tools/build_variant_fast.py): the kernels' memory / LDS traffic without their field arithmetic
#define fp_mul(a, b) ((a) ^ (b))
#define fp_add(a, b) ((a) + (b))
#define fp_sub(a, b) ((a) - (b))
#define fp_sub_lazy(a, b) ((a) - (b))
#endif
// measurement builds only: leave out one memory phase of the v4 / v5 kernels (results are then wrong, the timing shows what the phase costs)
//   1 twiddle-table fill   2 prescale loads   4 output-factor loads   8 global stores (kept alive by an impossible condition)   16 tile loads
#ifndef CS_NTT_SKIP
#define CS_NTT_SKIP 0
#endif

namespace cs {
namespace {

// The measurement hooks, kept out of the loops: in the product build (CS_NTT_SKIP == 0) mb_load is the load, mb_store the store, and
// the MB_* conditions are compile-time false.
__device__ __forceinline__ fp mb_load(const fp *row, unsigned lane_off, unsigned fake) { return (CS_NTT_SKIP & 16) ? (fp)fake : row[lane_off]; }
__device__ __forceinline__ void mb_store(fp *row, unsigned lane_off, fp val) {
    if (!(CS_NTT_SKIP & 8) || val == 0x123456789abcdefull) row[lane_off] = val; // (measurement: kept alive by an impossible condition)
}
constexpr bool MB_NO_TWIDDLE_FILL = (CS_NTT_SKIP & 1) != 0, MB_NO_PRESCALE = (CS_NTT_SKIP & 2) != 0, MB_NO_OUTPUT_FACTOR = (CS_NTT_SKIP & 4) != 0;

constexpr int NT = 256; // threads per workgroup

__device__ __forceinline__ unsigned bitrev(unsigned x, unsigned bits) { return __brev(x) >> (32 - bits); }

// In-LDS decimation-in-frequency transform of M = 2^log_m points for L interleaved sequences
// (element (i, l) at tile[i * L + l]).  Natural order in, bit-reversed positions out.
// tw[e] = w_M^e for e < M/2.  All NT threads of the workgroup take part.
template <int L>
__device__ __forceinline__ void lds_ntt_dif(fp *tile, unsigned log_m, const fp *tw) {
    const unsigned half_total = (1u << (log_m - 1)) * L;
    for (unsigned s = 0; s < log_m; s++) {
        const unsigned hbits = log_m - 1 - s, half = 1u << hbits;
        for (unsigned b = threadIdx.x; b < half_total; b += NT) {
            const unsigned l = b % L, q = b / L;
            const unsigned j = q & (half - 1);
            const unsigned i0 = ((q >> hbits) << (hbits + 1)) + j, i1 = i0 + half;
            const fp u = tile[i0 * L + l], v = tile[i1 * L + l];
            tile[i0 * L + l] = fp_add(u, v);
            tile[i1 * L + l] = fp_mul(fp_sub_lazy(u, v), tw[j << s]);
        }
        __syncthreads();
    }
}

// grid = (C / L, width, batch).  in/out column stride n; batch stride given explicitly.
template <int L>
__global__ __launch_bounds__(NT) void k_ntt_cols(const fp *__restrict__ in, fp *__restrict__ out, unsigned log_n, unsigned log_r,
                                                const fp *__restrict__ w, const fp *__restrict__ prescale, size_t in_batch_stride,
                                                size_t out_batch_stride, size_t prescale_batch_stride) {
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    const unsigned log_c = log_n - log_r, R = 1u << log_r;
    const size_t n = (size_t)1 << log_n;
    fp *tile = smem, *tw = smem + (size_t)R * L;
    const unsigned c0 = blockIdx.x * L;
    const fp *src = in + blockIdx.z * in_batch_stride + (size_t)blockIdx.y * n;
    fp *dst = out + blockIdx.z * out_batch_stride + (size_t)blockIdx.y * n;
    const fp *ps = prescale ? prescale + blockIdx.z * prescale_batch_stride : nullptr;

    for (unsigned e = threadIdx.x; e < R / 2; e += NT) tw[e] = w[(size_t)e << log_c];
    for (unsigned idx = threadIdx.x; idx < R * L; idx += NT) {
        const unsigned r = idx / L, l = idx % L;
        const size_t m = ((size_t)r << log_c) + c0 + l;
        fp v = src[m];
        if (ps) v = fp_mul(v, ps[m]);
        tile[idx] = v;
    }
    __syncthreads();
    lds_ntt_dif<L>(tile, log_r, tw);
    for (unsigned idx = threadIdx.x; idx < R * L; idx += NT) {
        const unsigned p = idx / L, l = idx % L;
        const unsigned k1 = bitrev(p, log_r), c = c0 + l;
        dst[((size_t)k1 << log_c) + c] = fp_mul(tile[idx], w[(size_t)k1 * c]);
    }
}

// grid = (R / L, width, batch).  in: rows [k1][c]; out: natural order k = k1 + R * k2.
template <int L>
__global__ __launch_bounds__(NT) void k_ntt_rows(const fp *__restrict__ in, fp *__restrict__ out, unsigned log_n, unsigned log_r,
                                                const fp *__restrict__ w, fp post_scale, int do_scale, size_t in_batch_stride,
                                                size_t out_batch_stride) {
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    const unsigned log_c = log_n - log_r, C = 1u << log_c;
    const size_t n = (size_t)1 << log_n;
    fp *tile = smem, *tw = smem + (size_t)C * L;
    const unsigned k10 = blockIdx.x * L;
    const fp *src = in + blockIdx.z * in_batch_stride + (size_t)blockIdx.y * n;
    fp *dst = out + blockIdx.z * out_batch_stride + (size_t)blockIdx.y * n;

    for (unsigned e = threadIdx.x; e < C / 2; e += NT) tw[e] = w[(size_t)e << log_r];
    for (unsigned c = threadIdx.x; c < C; c += NT) { // coalesced row reads, transposed into [c][l] through registers
        fp v[L];
#pragma unroll
        for (int l = 0; l < L; l++) v[l] = src[((size_t)(k10 + l) << log_c) + c];
#pragma unroll
        for (int l = 0; l < L; l++) tile[c * L + l] = v[l];
    }
    __syncthreads();
    lds_ntt_dif<L>(tile, log_c, tw);
    for (unsigned idx = threadIdx.x; idx < C * L; idx += NT) {
        const unsigned p = idx / L, l = idx % L;
        const unsigned k2 = bitrev(p, log_c);
        fp v = tile[idx];
        if (do_scale) v = fp_mul(v, post_scale);
        dst[((size_t)k2 << log_r) + k10 + l] = v;
    }
}

// =====================================================================================================
// Register kernels for the three product sizes 2^16, 2^18 and 2^20 (three_step_size below): the same two passes with every
// 2^LOGM-point sub-transform in THREE register steps of 2^LA, 2^LB and 2^LC points (LA >= LB >= LC; compile-time twiddles, fully
// unrolled) and an exchange through LDS between two steps.  L2 = 8 adjacent columns / rows per workgroup make every global access a
// 64-byte segment.  A thread holds 2^LA <= 16 elements, and a CU holds four waves per SIMD or more: the two-step kernels these replaced
// (32 elements per thread, two waves per SIMD) spent half of their wave cycles waiting (rocprofv3: SQ_WAIT_ANY 22-39 %,
// SQ_WAIT_INST_ANY 16-30 % of SQ_WAVE_CYCLES) because two waves per SIMD cannot cover global-load latency, LDS round trips and the
// issue gaps of dependent v_mad_u64_u32 chains.
//
// Index algebra (w = w_M, M = 2^LOGM, T = 2^(LB+LC)):  r = r1 T + r2 2^LC + r3,  k = k1 + 2^LA k2 + 2^(LA+LB) k3
//   step 1  (r2, r3) fixed: Y[k1]  = sum_r1 x[r] w_{2^LA}^(r1 k1),  then  * w^((r2 2^LC + r3) k1)
//   step 2  (k1, r3) fixed: Z[k2]  = sum_r2 Y[k1; r2, r3] w_{2^LB}^(r2 k2),  then  * w^(2^LA r3 k2)
//   step 3  (k1, k2) fixed: X[k3]  = sum_r3 Z[k1, k2; r3] w_{2^LC}^(r3 k3)
// LDS tile: element (k1, q, l) at (k1 T + q) L2 + l (columns kernel) resp. ((k1 L2 + l)(T + 4) + q) (rows kernel), q = r2 2^LC + r3
// after step 1; step 2 works in place and stores Z[k2] of task (k1, r3) at q = k2 2^LC + (r3 ^ (k2 mod 2^LC)) so that step 3's
// reads (fixed r3, lanes over k2) fall into distinct banks.
// -----------------------------------------------------------------------------------------------------
// compile-time field arithmetic for the small twiddle tables
__host__ __device__ constexpr uint64_t cx_mul(uint64_t a, uint64_t b) {
    unsigned __int128 t = (unsigned __int128)a * b;
    uint64_t m = (uint64_t)t * 0x417fffffffffffffULL;
    uint64_t r = (uint64_t)((t + (unsigned __int128)m * FP_P) >> 64);
    return r >= FP_P ? r - FP_P : r;
}
__host__ __device__ constexpr uint64_t cx_pow(uint64_t b, uint64_t e) {
    uint64_t r = FP_ONE;
    while (e) { if (e & 1) r = cx_mul(r, b); b = cx_mul(b, b); e >>= 1; }
    return r;
}
// w_{2^log}^k (INV: its inverse); 2^55-th root of unity = generator^131 [UPSTREAM-RECALL, include/cstark_conventions.h, same as hostfield.h]
__host__ __device__ constexpr uint64_t cx_root(int log, bool inv) {
    uint64_t g = cx_pow(cx_mul(CSTARK_CONV_FIELD_GENERATOR, FP_R2), CSTARK_CONV_TWO_ADIC_ROOT_EXP);
    for (int i = log; i < 55; i++) g = cx_mul(g, g);
    return inv ? cx_pow(g, FP_P - 2) : g;
}
template <int LOG, bool INV>
struct SmallTw {
    uint64_t v[LOG == 0 ? 1 : (1 << LOG) / 2 + 1];
    constexpr SmallTw() : v{} {
        const uint64_t w = cx_root(LOG, INV);
        uint64_t x = FP_ONE;
        for (int i = 0; i < (1 << LOG) / 2 + (LOG == 0); i++) { v[i] = x; x = cx_mul(x, w); }
    }
};

// 2^LOG-point DIF transform in registers: natural order in, x[p] = X[bitrev(p)] out
template <int LOG, bool INV>
__device__ __forceinline__ void reg_ntt_dif(fp (&x)[1 << LOG]) {
    constexpr SmallTw<LOG, INV> tw{};
    constexpr int N = 1 << LOG;
#pragma unroll
    for (int s = 0; s < LOG; s++) {
        const int half = N >> (s + 1);
#pragma unroll
        for (int blk = 0; blk < (1 << s); blk++) {
#pragma unroll
            for (int j = 0; j < half; j++) {
                const int i0 = blk * 2 * half + j, i1 = i0 + half;
                const fp u = x[i0], v = x[i1];
                x[i0] = fp_add(u, v);
                x[i1] = (j == 0) ? fp_sub(u, v) : fp_mul(fp_sub_lazy(u, v), tw.v[j << s]); // the product takes a first factor < 2p
            }
        }
    }
}
__host__ __device__ constexpr unsigned cx_brev(unsigned x, int bits) {
    unsigned r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}

constexpr int L2 = 8; // columns / rows per workgroup of the register kernels: 64-byte global segments, and the tile of the largest size fits 64 KB of LDS
// Workgroups are dealt to the 8 XCDs round-robin by linear id, and each XCD has its own L2.  With 64-byte tiles two
// neighbouring tiles share every 128-byte line, so neighbours are given ids 8 apart: same XCD, dispatched back to back.
// (The tile counts of the three-step sizes are multiples of 16.)
__device__ __forceinline__ unsigned xcd_pair_tile(unsigned y) { return (y & ~15u) | ((y & 7u) << 1) | ((y >> 3) & 1u); }

template <int LA, int LB, int LC>
struct V4 {
    static constexpr int A = 1 << LA, Bn = 1 << LB, Cn = 1 << LC, T = Bn * Cn, M = A * T, LOGM = LA + LB + LC;
    static constexpr int NT = L2 * T;       // threads per workgroup: one step-1 task each
    static constexpr int J2 = A / Bn;       // step-2 tasks (k1, r3) per thread
    static constexpr int J3 = A / Cn;       // step-3 tasks (k1, k2) per thread
    static_assert(LA >= LB && LB >= LC && LC >= 1, "step sizes must not increase");
};
// One workgroup works on ONE tile.  Measured on MI355X (2^20 x 94 x 8) and dropped: several tiles per workgroup with the next tile's
// global loads issued before the current tile's arithmetic -- the register prefetch pushes hipcc past the 128 VGPRs that four waves
// per SIMD allow (15-34 spilled registers even behind scheduling barriers) and the extension takes 11.2 instead of 8.6 ms.  Also
// measured and dropped: steps 2 and 3 task by task inside one wave (the 64 lanes of a wave are the L2 columns x the 8 tasks of one
// k1, so no workgroup barrier is needed after step 1) -- 9.2 ms: the per-task LDS round trips serialise; all cosets of a tile in one
// workgroup with the coefficients kept in registers -- 83 spilled registers.

// ---- the parts of a three-step pass, written as helpers.  Only the v5 kernels use them: the v4 kernels keep copies of their own, see their note
// tw[e] = w_M^e, e < M, from the dense table of the pass (NttAux); all threads of the workgroup take part
template <int LA, int LB, int LC>
__device__ __forceinline__ void fill_twiddles(fp *tw, const fp *__restrict__ tab) {
    using G = V4<LA, LB, LC>;
    if (MB_NO_TWIDDLE_FILL) { for (unsigned e = threadIdx.x; e < G::M; e += G::NT) tw[e] = e; }
    else for (unsigned e = threadIdx.x; e < G::M; e += G::NT) tw[e] = tab[e];
}

// The dense side tables of the column pass (ntt_build_aux_*), M = 2^log_r points per sub-transform, C = 2^log_c columns:
//   aux               = [M] twiddles of this pass | [C] twiddles of the row pass | [C] ratios w_n^(A Bn c) | [A Bn][C] output factors w_n^(kb c)
//   aux_ps (per coset) = [M] row part shift^(r C) of the prescale | [A Bn][C] output factors times the column part shift^c
// aux_ps == nullptr: a transform without prescale.
struct ColsTables { const fp *ps_row, *outf, *ratio; };
template <int LA, int LB, int LC>
__device__ __forceinline__ ColsTables cols_tables(const fp *__restrict__ aux, const fp *__restrict__ aux_ps, size_t aux_ps_batch_stride, unsigned bz,
                                                  unsigned log_c) {
    constexpr int M = V4<LA, LB, LC>::M;
    ColsTables tb;
    tb.ps_row = aux_ps ? aux_ps + bz * aux_ps_batch_stride : nullptr;
    tb.outf = tb.ps_row ? tb.ps_row + M : aux + M + ((size_t)2 << log_c);
    tb.ratio = aux + M + ((size_t)1 << log_c);
    return tb;
}

// Step 1's inputs of the column pass: rows r = r1 T + t of column c, times the row part shift^(r C) of the coset power (the column
// part shift^c is folded into the output factor)
template <int LA, int LB, int LC>
__device__ __forceinline__ void cols_load_prescaled(fp (&a)[1 << LA], const fp *__restrict__ src, const fp *__restrict__ ps_row, unsigned log_c, unsigned t,
                                                    unsigned c) {
    constexpr int A = V4<LA, LB, LC>::A, T = V4<LA, LB, LC>::T;
    const unsigned lane_off = (t << log_c) + c; // uniform row base + 32-bit lane offset: one address register for all loads
#pragma unroll
    for (int r1 = 0; r1 < A; r1++) a[r1] = mb_load(src + ((size_t)(r1 * T) << log_c), lane_off, lane_off + r1);
    if (!MB_NO_PRESCALE && ps_row) {
#pragma unroll
        for (int r1 = 0; r1 < A; r1++) a[r1] = fp_mul(a[r1], ps_row[r1 * T + t]);
    }
}

// The column pass's epilogue for one step-3 task (kb = k1 + A k2, column c): x[] holds X[k3] in bit-reversed positions; output rows
// k = kb + A Bn k3 take the factor shift^c w_n^(k c), a geometric sequence in k3 with ratio w_n^(A Bn c).  First factor and ratio come
// from the dense tables: one 64-byte segment per (kb, tile) instead of 8 scattered sectors of the n-entry table.
template <int LA, int LB, int LC>
__device__ __forceinline__ void cols_store_task(const fp (&x)[1 << LC], unsigned kb, unsigned c, unsigned log_c, const ColsTables &tb, fp *__restrict__ dst) {
    constexpr int A = V4<LA, LB, LC>::A, Bn = V4<LA, LB, LC>::Bn, Cn = V4<LA, LB, LC>::Cn;
    fp g, ratio;
    if (MB_NO_OUTPUT_FACTOR) { g = kb + c; ratio = c; }
    else { g = tb.outf[((size_t)kb << log_c) + c]; ratio = tb.ratio[c]; }
    const unsigned lane_off = (kb << log_c) + c; // uniform row base + 32-bit lane offset: one address register for all stores
#pragma unroll
    for (int k3 = 0; k3 < Cn; k3++) {
        fp *row = dst + ((size_t)(A * Bn * k3) << log_c);
        const fp val = fp_mul(x[cx_brev(k3, LC)], g);
        mb_store(row, lane_off, val);
        if (k3 + 1 < Cn) g = fp_mul(g, ratio);
    }
}

// The row pass's step-3 stores for one task (kb = j1 + A j2, row l of the tile at dst_tile): x[p] = X[j3 = brev(p)] goes to output
// frequency k2 = kb + A Bn j3, the transposition back to natural order
template <int LA, int LB, int LC>
__device__ __forceinline__ void rows_store_task(const fp (&x)[1 << LC], unsigned kb, unsigned l, unsigned log_r, fp post_scale, int do_scale,
                                                fp *__restrict__ dst_tile) {
    constexpr int A = V4<LA, LB, LC>::A, Bn = V4<LA, LB, LC>::Bn, Cn = V4<LA, LB, LC>::Cn;
    const unsigned out_lane = (kb << log_r) + l;
#pragma unroll
    for (int p = 0; p < Cn; p++) {
        fp val = x[p];
        if (do_scale) val = fp_mul(val, post_scale);
        mb_store(dst_tile + ((size_t)(A * Bn * cx_brev(p, LC)) << log_r), out_lane, val);
    }
}

// Step 1's inputs of the row pass of a STEP column (see "step columns" below): the thread's row `rows` (in_lane: its 32-bit lane offset)
// is a row of the per-coset table W, and entry c = c1 T + s1 takes the column's factor A[c mod 2^log_t] (fac_mask = 2^log_t - 1) on
// its way in -- the product is formed at the load, the 2^LA values are the only live state
template <int LA, int LB, int LC>
__device__ __forceinline__ void rows_load_step(fp (&a)[1 << LA], const fp *__restrict__ rows, unsigned in_lane, unsigned s1, const fp *__restrict__ fac,
                                               unsigned fac_mask) {
    constexpr int A = V4<LA, LB, LC>::A, T = V4<LA, LB, LC>::T;
#pragma unroll
    for (int c1 = 0; c1 < A; c1++) a[c1] = mb_load(rows + c1 * T, in_lane, in_lane + c1);
#pragma unroll
    for (int c1 = 0; c1 < A; c1++) a[c1] = fp_mul(a[c1], fac[(c1 * T + s1) & fac_mask]);
}
// The same for a TWO-LEVEL column (see "two-level columns" below): the sum of two such products, rows * fac + rows_r * fac_r, with the
// thread's row of the second table W_R and the column's second factors A2
template <int LA, int LB, int LC>
__device__ __forceinline__ void rows_load_step2(fp (&a)[1 << LA], const fp *__restrict__ rows, const fp *__restrict__ rows_r, unsigned in_lane, unsigned s1,
                                                const fp *__restrict__ fac, const fp *__restrict__ fac_r, unsigned fac_mask) {
    constexpr int A = V4<LA, LB, LC>::A, T = V4<LA, LB, LC>::T;
    // One entry at a time: left to the scheduler, all 2^(LA+2) loads of a thread are issued first and the 2^20 kernel spills (80 VGPRs at six
    // waves per SIMD; 60 dwords of scratch, and still 18 with two entries at a time).  The tables are read-only memory, whose loads no fence holds
    // back, so the next entry's offsets are made to depend on this entry's sum.  64 VGPRs, no scratch; the waves of the other workgroups of a
    // CU cover the serial round trips.
    unsigned off = in_lane, sv = s1;
#pragma unroll
    for (int c1 = 0; c1 < A; c1++) {
        const fp w = mb_load(rows + c1 * T, off, off + c1), wr = mb_load(rows_r + c1 * T, off, off + c1);
        const unsigned j = (c1 * T + sv) & fac_mask;
        a[c1] = fp_add(fp_mul(w, fac[j]), fp_mul(wr, fac_r[j]));
        if (c1 + 1 < A) asm volatile("" : "+v"(off), "+v"(sv) : "v"((unsigned)a[c1]));
    }
}

// ---- v4: whole-tile exchanges ------------------------------------------------------------------------------------------------------
// k_ntt_cols_v4, k_ntt_rows_v4 and cols_v4_finish below still carry what the v5 kernels have shed: the table-less fallbacks behind
// `aux == nullptr` (no caller reaches them: launch_three_step refuses a size without its tables) and the shape of the multi-tile
// prefetch loop, run for one tile.  Rewritten onto the helpers above they compute the same and time the same alone, but SchnorrAir's
// 2^18 proof, which runs narrow transforms next to the trace kernels of a second stream, measured 0.2 ms slower, and neither the
// barrier positions nor the loop's scheduling barrier explained it (profiles/ntt_generations_ab.txt).  Until the cause is known they
// keep this text.
constexpr int V4_TILES = 1;


// Steps 2 and 3 of the column pass on the tile in LDS (after step 1 stored Y * twiddle), including the output factor and the
// stores.  t, l: this thread's position; kb-dependent factors from w / ps where the dense tables are absent.
template <int LA, int LB, int LC, bool INV>
__device__ __forceinline__ void cols_v4_finish(fp *tile, const fp *tw, const fp *__restrict__ w, const fp *__restrict__ ps, fp *__restrict__ dst,
                                               unsigned log_c, unsigned c, unsigned t, unsigned l, const fp *__restrict__ outf,
                                               const fp *__restrict__ ratio_tab) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T;
    fp z[G::J2][Bn];
#pragma unroll
    for (int j = 0; j < G::J2; j++) { // step 2: task u = t + T j = k1 Cn + r3
        const unsigned u = t + T * j, k1 = u / Cn, r3 = u % Cn;
#pragma unroll
        for (int r2 = 0; r2 < Bn; r2++) z[j][r2] = tile[((size_t)k1 * T + r2 * Cn + r3) * L2 + l];
    }
    __syncthreads(); // every input of step 2 is in registers: the tile can be overwritten
#pragma unroll
    for (int j = 0; j < G::J2; j++) {
        const unsigned u = t + T * j, k1 = u / Cn, r3 = u % Cn;
        reg_ntt_dif<LB, INV>(z[j]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned k2 = cx_brev(p, LB);
            const fp v = (k2 == 0) ? z[j][p] : fp_mul(z[j][p], tw[(A * k2) * r3]);
            tile[((size_t)k1 * T + k2 * Cn + (r3 ^ (k2 % Cn))) * L2 + l] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G::J3; j++) { // step 3: task v = t + T j = k1 Bn + k2; output rows k = k1 + A k2 + A Bn k3
        const unsigned v = t + T * j, k1 = v / Bn, k2 = v % Bn;
        fp x[Cn];
#pragma unroll
        for (int r3 = 0; r3 < Cn; r3++) x[r3] = tile[((size_t)k1 * T + k2 * Cn + (r3 ^ (k2 % Cn))) * L2 + l];
        reg_ntt_dif<LC, INV>(x);
        // output factor shift^c w_n^(k c), k = (k1 + A k2) + A Bn k3: a geometric sequence in k3 with ratio w_n^(A Bn c)
        const unsigned kb = k1 + A * k2;
        fp g, ratio;
        if (MB_NO_OUTPUT_FACTOR) { g = kb + c; ratio = c; }
        else if (outf) { // compact tables (ntt_build_aux_*): one 64-byte segment per (kb, tile) instead of 8 scattered sectors
            g = outf[((size_t)kb << log_c) + c];
            ratio = ratio_tab[c];
        } else {
            g = w[(size_t)kb * c];
            if (ps) g = fp_mul(g, ps[c]);
            ratio = w[(size_t)(A * Bn) * c];
        }
        const unsigned lane_off = (kb << log_c) + c; // uniform row base + 32-bit lane offset: one address register for all stores
#pragma unroll
        for (int k3 = 0; k3 < Cn; k3++) {
            fp *row = dst + ((size_t)(A * Bn * k3) << log_c);
            const fp val = fp_mul(x[cx_brev(k3, LC)], g);
            mb_store(row, lane_off, val);
            if (k3 + 1 < Cn) g = fp_mul(g, ratio);
        }
    }
}

// grid = (C / L2 / V4_TILES, batch, width)
template <int LA, int LB, int LC, bool INV>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), 4) void k_ntt_cols_v4(const fp *__restrict__ in, fp *__restrict__ out, unsigned log_n,
                                                                        const fp *__restrict__ w, const fp *__restrict__ prescale,
                                                                        size_t in_batch_stride, size_t out_batch_stride, size_t prescale_batch_stride,
                                                                        const fp *__restrict__ aux, const fp *__restrict__ aux_ps,
                                                                        size_t aux_ps_batch_stride) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, T = G::T, M = G::M, LOGM = G::LOGM;
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                      // [A][T][L2]
    fp *tw = smem + (size_t)M * L2;       // [M] powers of w_M
    const unsigned log_c = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const unsigned bz = blockIdx.y, tile_id = blockIdx.x; // batch (coset), tile: see the grid note at k_ntt_cols_v5
    const fp *src = in + bz * in_batch_stride + (size_t)blockIdx.z * n;
    fp *dst = out + bz * out_batch_stride + (size_t)blockIdx.z * n;
    const fp *ps = prescale ? prescale + bz * prescale_batch_stride : nullptr;
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2;
    // compact tables (NttAux): aux = [M] twiddles of this pass | [C] twiddles of the row pass | [C] ratios | [A Bn][C] output factors;
    // aux_ps (per batch) = [M] row part of the prescale | [A Bn][C] output factors times the column part
    const fp *ps_row = (ps && aux_ps) ? aux_ps + bz * aux_ps_batch_stride : nullptr;
    const fp *outf = !aux ? nullptr : ps ? (ps_row ? ps_row + M : nullptr) : aux + M + ((size_t)2 << log_c);
    const fp *ratio_tab = aux ? aux + M + ((size_t)1 << log_c) : nullptr;

    if (MB_NO_TWIDDLE_FILL) { for (unsigned e = threadIdx.x; e < M; e += G::NT) tw[e] = e; }
    else if (aux) for (unsigned e = threadIdx.x; e < M; e += G::NT) tw[e] = aux[e];
    else for (unsigned e = threadIdx.x; e < M; e += G::NT) tw[e] = w[(size_t)e << log_c];
    fp nxt[A];
    {
        const unsigned lane_off = (t << log_c) + xcd_pair_tile(tile_id * V4_TILES) * L2 + l;
#pragma unroll
        for (int r1 = 0; r1 < A; r1++) nxt[r1] = mb_load(src + ((size_t)(r1 * T) << log_c), lane_off, lane_off + r1);
    }
    __syncthreads(); // tw[] ready
#pragma unroll 1
    for (int it = 0; it < V4_TILES; it++) {
        const unsigned c = xcd_pair_tile(tile_id * V4_TILES + it) * L2 + l;
        {   // step 1: rows r = r1 T + t
            fp a[A];
#pragma unroll
            for (int r1 = 0; r1 < A; r1++) a[r1] = nxt[r1];
            if (it + 1 < V4_TILES) {
                const unsigned lane_off = (t << log_c) + xcd_pair_tile(tile_id * V4_TILES + it + 1) * L2 + l;
#pragma unroll
                for (int r1 = 0; r1 < A; r1++) nxt[r1] = (src + ((size_t)(r1 * T) << log_c))[lane_off];
            }
            __builtin_amdgcn_sched_barrier(0); // the prefetch is issued here, ahead of this tile's arithmetic
            if (MB_NO_PRESCALE) {
            } else if (ps_row) { // row part shift^(r C) of the coset power; the column part shift^c is folded into the output factor
#pragma unroll
                for (int r1 = 0; r1 < A; r1++) a[r1] = fp_mul(a[r1], ps_row[r1 * T + t]);
            } else if (ps) {
                const unsigned ps_off = t << log_c;
#pragma unroll
                for (int r1 = 0; r1 < A; r1++) a[r1] = fp_mul(a[r1], (ps + ((size_t)(r1 * T) << log_c))[ps_off]);
            }
            reg_ntt_dif<LA, INV>(a);
#pragma unroll
            for (int p = 0; p < A; p++) {
                const unsigned k1 = cx_brev(p, LA);
                tile[((size_t)k1 * T + t) * L2 + l] = (k1 == 0) ? a[p] : fp_mul(a[p], tw[k1 * t]);
            }
        }
        __syncthreads();
        cols_v4_finish<LA, LB, LC, INV>(tile, tw, w, ps, dst, log_c, c, t, l, outf, ratio_tab);
        __syncthreads(); // the tile is rewritten by the next iteration
    }
}

// grid = (batch, R / L2 / V4_TILES, width).  in: rows [k1][c] (each row M contiguous); out: natural order k = k1 + R * k2.
template <int LA, int LB, int LC, bool INV>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), 4) void k_ntt_rows_v4(const fp *__restrict__ in, fp *__restrict__ out, unsigned log_n,
                                                                        const fp *__restrict__ w, fp post_scale, int do_scale,
                                                                        size_t in_batch_stride, size_t out_batch_stride, const fp *__restrict__ aux_tw) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, M = G::M, LOGM = G::LOGM;
    constexpr int TP = T + 4; // padded run of q per (j1, l): lanes over l then hit distinct banks (T + 4 = 4 mod 32 for T = 32, 64)
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                              // [A][L2][TP]
    fp *tw = smem + (size_t)A * L2 * TP;          // [M]
    const unsigned log_r = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const fp *src = in + blockIdx.x * in_batch_stride + (size_t)blockIdx.z * n;
    fp *dst = out + blockIdx.x * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned s1 = threadIdx.x % T, l1 = threadIdx.x / T; // step 1: s = c2 Cn + c3 fastest across lanes (coalesced row reads)
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2; // steps 2 and 3: l fastest across lanes (64-byte transposed stores)

    if (MB_NO_TWIDDLE_FILL) { for (unsigned e = threadIdx.x; e < M; e += G::NT) tw[e] = e; }
    else if (aux_tw) for (unsigned e = threadIdx.x; e < M; e += G::NT) tw[e] = aux_tw[e];
    else for (unsigned e = threadIdx.x; e < M; e += G::NT) tw[e] = w[(size_t)e << log_r];
    fp nxt[A];
    const unsigned in_lane = (l1 << LOGM) + s1; // uniform row base + 32-bit lane offset: one address register for all loads
    {
        const unsigned k10 = xcd_pair_tile(blockIdx.y * V4_TILES) * L2;
#pragma unroll
        for (int c1 = 0; c1 < A; c1++) nxt[c1] = mb_load(src + ((size_t)k10 << LOGM) + c1 * T, in_lane, in_lane + c1);
    }
    __syncthreads(); // tw[] ready
#pragma unroll 1
    for (int it = 0; it < V4_TILES; it++) {
        const unsigned k10 = xcd_pair_tile(blockIdx.y * V4_TILES + it) * L2;
        {   // step 1: columns c = c1 T + s
            fp a[A];
#pragma unroll
            for (int c1 = 0; c1 < A; c1++) a[c1] = nxt[c1];
            if (it + 1 < V4_TILES) {
                const unsigned k11 = xcd_pair_tile(blockIdx.y * V4_TILES + it + 1) * L2;
#pragma unroll
                for (int c1 = 0; c1 < A; c1++) nxt[c1] = (src + ((size_t)k11 << LOGM) + c1 * T)[in_lane];
            }
            __builtin_amdgcn_sched_barrier(0); // the prefetch is issued here, ahead of this tile's arithmetic
            reg_ntt_dif<LA, INV>(a);
#pragma unroll
            for (int p = 0; p < A; p++) {
                const unsigned j1 = cx_brev(p, LA);
                tile[((size_t)j1 * L2 + l1) * TP + s1] = (j1 == 0) ? a[p] : fp_mul(a[p], tw[j1 * s1]);
            }
        }
        __syncthreads();
        fp z[G::J2][Bn];
#pragma unroll
        for (int j = 0; j < G::J2; j++) { // step 2: task u = t + T j = j1 Cn + c3
            const unsigned u = t + T * j, j1 = u / Cn, c3 = u % Cn;
#pragma unroll
            for (int c2 = 0; c2 < Bn; c2++) z[j][c2] = tile[((size_t)j1 * L2 + l) * TP + c2 * Cn + c3];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < G::J2; j++) {
            const unsigned u = t + T * j, j1 = u / Cn, c3 = u % Cn;
            reg_ntt_dif<LB, INV>(z[j]);
#pragma unroll
            for (int p = 0; p < Bn; p++) {
                const unsigned j2 = cx_brev(p, LB);
                const fp v = (j2 == 0) ? z[j][p] : fp_mul(z[j][p], tw[(A * j2) * c3]);
                tile[((size_t)j1 * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < G::J3; j++) { // step 3: task v = t + T j = j1 Bn + j2; output frequency k2 = j1 + A j2 + A Bn j3
            const unsigned v = t + T * j, j1 = v / Bn, j2 = v % Bn;
            fp x[Cn];
#pragma unroll
            for (int c3 = 0; c3 < Cn; c3++) x[c3] = tile[((size_t)j1 * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))];
            reg_ntt_dif<LC, INV>(x);
            const unsigned out_lane = ((j1 + A * j2) << log_r) + l;
#pragma unroll
            for (int p = 0; p < Cn; p++) {
                fp val = x[p];
                if (do_scale) val = fp_mul(val, post_scale);
                mb_store(dst + ((size_t)(A * Bn * cx_brev(p, LC)) << log_r) + k10, out_lane, val);
            }
        }
        __syncthreads(); // the tile is rewritten by the next iteration
    }
}

// The same pass for step columns (rows_load_step): batch b reads wtab [b][n] (ntt_step_build_tables), column z takes the factors fac [z][2^log_t].
// Written on the helpers, one tile per workgroup and dense tables only -- k_ntt_rows_v4 keeps its own text, see the note above: as a
// shared body it compiles to other register figures (2^18: 39 instead of 40 VGPRs; 2^16: 42 instead of 32 SGPRs).
template <int LA, int LB, int LC>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), 4) void k_ntt_rows_step_v4(const fp *__restrict__ wtab, const fp *__restrict__ fac, fp *__restrict__ out,
                                                                             unsigned log_n, unsigned log_t, size_t out_batch_stride,
                                                                             const fp *__restrict__ aux_tw) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, LOGM = G::LOGM;
    constexpr int TP = T + 4;
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                              // [A][L2][TP]
    fp *tw = smem + (size_t)A * L2 * TP;          // [M]
    const unsigned log_r = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const fp *src = wtab + blockIdx.x * n;
    fp *dst = out + blockIdx.x * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned s1 = threadIdx.x % T, l1 = threadIdx.x / T;
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2;
    const unsigned k10 = xcd_pair_tile(blockIdx.y) * L2;
    fp a[A];
    rows_load_step<LA, LB, LC>(a, src + ((size_t)k10 << LOGM), (l1 << LOGM) + s1, s1, fac + ((size_t)blockIdx.z << log_t), (1u << log_t) - 1);
    fill_twiddles<LA, LB, LC>(tw, aux_tw);
    reg_ntt_dif<LA, false>(a); // step 1: columns c = c1 T + s
    __syncthreads(); // tw[] ready
#pragma unroll
    for (int p = 0; p < A; p++) {
        const unsigned j1 = cx_brev(p, LA);
        tile[((size_t)j1 * L2 + l1) * TP + s1] = (j1 == 0) ? a[p] : fp_mul(a[p], tw[j1 * s1]);
    }
    __syncthreads();
    fp z[G::J2][Bn];
#pragma unroll
    for (int j = 0; j < G::J2; j++) { // step 2: task u = t + T j = j1 Cn + c3
        const unsigned u = t + T * j, j1 = u / Cn, c3 = u % Cn;
#pragma unroll
        for (int c2 = 0; c2 < Bn; c2++) z[j][c2] = tile[((size_t)j1 * L2 + l) * TP + c2 * Cn + c3];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G::J2; j++) {
        const unsigned u = t + T * j, j1 = u / Cn, c3 = u % Cn;
        reg_ntt_dif<LB, false>(z[j]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned j2 = cx_brev(p, LB);
            tile[((size_t)j1 * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))] = (j2 == 0) ? z[j][p] : fp_mul(z[j][p], tw[(A * j2) * c3]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G::J3; j++) { // step 3: task v = t + T j = j1 Bn + j2
        const unsigned v = t + T * j, j1 = v / Bn, j2 = v % Bn;
        fp x[Cn];
#pragma unroll
        for (int c3 = 0; c3 < Cn; c3++) x[c3] = tile[((size_t)j1 * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))];
        reg_ntt_dif<LC, false>(x);
        rows_store_task<LA, LB, LC>(x, j1 + A * j2, l, log_r, 0, 0, dst + k10);
    }
}

// k_ntt_rows_step_v4 for two-level columns (rows_load_step2): wtab_r [b][n] is the second table, fac [z][2][2^log_t] the factors A1 | A2.  Its own
// text for the reason above: a load selected by a template parameter would be a shared body again.
template <int LA, int LB, int LC>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), 4) void k_ntt_rows_step2_v4(const fp *__restrict__ wtab, const fp *__restrict__ wtab_r, const fp *__restrict__ fac,
                                                                              fp *__restrict__ out, unsigned log_n, unsigned log_t, size_t out_batch_stride,
                                                                              const fp *__restrict__ aux_tw) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, LOGM = G::LOGM;
    constexpr int TP = T + 4;
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                              // [A][L2][TP]
    fp *tw = smem + (size_t)A * L2 * TP;          // [M]
    const unsigned log_r = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const fp *src = wtab + blockIdx.x * n;
    const fp *src_r = wtab_r + blockIdx.x * n;
    const fp *fac_z = fac + ((size_t)blockIdx.z << (log_t + 1)); // A1 [T] | A2 [T]
    fp *dst = out + blockIdx.x * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned s1 = threadIdx.x % T, l1 = threadIdx.x / T;
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2;
    const unsigned k10 = xcd_pair_tile(blockIdx.y) * L2;
    fp a[A];
    rows_load_step2<LA, LB, LC>(a, src + ((size_t)k10 << LOGM), src_r + ((size_t)k10 << LOGM), (l1 << LOGM) + s1, s1, fac_z, fac_z + ((size_t)1 << log_t),
                                (1u << log_t) - 1);
    fill_twiddles<LA, LB, LC>(tw, aux_tw);
    reg_ntt_dif<LA, false>(a); // step 1: columns c = c1 T + s
    __syncthreads(); // tw[] ready
#pragma unroll
    for (int p = 0; p < A; p++) {
        const unsigned j1 = cx_brev(p, LA);
        tile[((size_t)j1 * L2 + l1) * TP + s1] = (j1 == 0) ? a[p] : fp_mul(a[p], tw[j1 * s1]);
    }
    __syncthreads();
    fp z[G::J2][Bn];
#pragma unroll
    for (int j = 0; j < G::J2; j++) { // step 2: task u = t + T j = j1 Cn + c3
        const unsigned u = t + T * j, j1 = u / Cn, c3 = u % Cn;
#pragma unroll
        for (int c2 = 0; c2 < Bn; c2++) z[j][c2] = tile[((size_t)j1 * L2 + l) * TP + c2 * Cn + c3];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G::J2; j++) {
        const unsigned u = t + T * j, j1 = u / Cn, c3 = u % Cn;
        reg_ntt_dif<LB, false>(z[j]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned j2 = cx_brev(p, LB);
            tile[((size_t)j1 * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))] = (j2 == 0) ? z[j][p] : fp_mul(z[j][p], tw[(A * j2) * c3]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G::J3; j++) { // step 3: task v = t + T j = j1 Bn + j2
        const unsigned v = t + T * j, j1 = v / Bn, j2 = v % Bn;
        fp x[Cn];
#pragma unroll
        for (int c3 = 0; c3 < Cn; c3++) x[c3] = tile[((size_t)j1 * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))];
        reg_ntt_dif<LC, false>(x);
        rows_store_task<LA, LB, LC>(x, j1 + A * j2, l, log_r, 0, 0, dst + k10);
    }
}

// =====================================================================================================
// v5 kernels: the v4 passes for shapes with two step-2 and two step-3 tasks per thread (2^LA = 2 * 2^LB = 2 * 2^LC: the
// 16 * 8 * 8 split of 1024 points), with each of the two exchanges done in TWO HALVES through a tile of half the size.  The tasks
// of a thread are task h = 0, 1 with k1 in [8 h, 8 h + 8): step 1 writes its eight outputs of half h, every thread reads the
// inputs of its task h, then the same buffer takes the other half.  32 KB of tile + 8 KB of twiddles per workgroup instead of
// 72: LDS no longer limits residency (registers do: three workgroups per CU in the row pass, two in the column pass), so a CU holds workgroups in
// different phases -- the loads and stores of one run under the arithmetic of the others.  (v4 measured with its arithmetic
// alone 5.55 ms, with its memory traffic alone 5.74 ms, together 8.0 ms for 94 columns x 8 cosets: two resident workgroups
// overlap too little.)  Register need after the cheaper field product: 62 (rows) / 95 (columns) VGPRs.
// -----------------------------------------------------------------------------------------------------
constexpr int V5_COLS_WAVES = 5; // 95 VGPRs, no spills, two workgroups per CU; 6 (80 VGPRs, 8 spilled -> 30 % more HBM writes): LDE 7.80 vs 7.58 ms
constexpr int V5_ROWS_WAVES = 6; // 62 VGPRs fit: three workgroups per CU
// The row pass, too, takes one tile per workgroup.  Measured (94 columns x 8 cosets) and dropped: the next tile's loads issued once the
// first exchange has freed the data registers -- 1 tile, three workgroups per CU 7.85 ms; 4 tiles at four waves per SIMD (128 VGPRs,
// 2 spilled) 8.27 ms; 2 tiles (16 spilled) 8.77 ms: more resident workgroups beat the software prefetch again.
template <int LA, int LB, int LC, bool INV>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), V5_COLS_WAVES) void k_ntt_cols_v5(const fp *__restrict__ in, fp *__restrict__ out, unsigned log_n,
                                                                                    size_t in_batch_stride, size_t out_batch_stride,
                                                                                    const fp *__restrict__ aux, const fp *__restrict__ aux_ps,
                                                                                    size_t aux_ps_batch_stride) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, M = G::M, LOGM = G::LOGM, AH = A / 2;
    static_assert(G::J2 == 2 && G::J3 == 2 && Bn == AH && Cn == AH, "two tasks per thread and step, one per half");
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                        // [A / 2][T][L2]
    fp *tw = smem + (size_t)(M / 2) * L2;   // [M] powers of w_M
    const unsigned log_c = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    // grid = (C / L2, batch, width): the TILE is the fastest grid dimension.  Workgroups go to the 8 XCDs round-robin by linear id, so
    // the XCD of a workgroup is its tile index mod 8 whatever its coset: the eight cosets of a tile -- which read the SAME coefficients
    // -- share one L2, and the coefficient table leaves HBM once per extension instead of once per coset (round 2: batch fastest put
    // coset k on XCD k, and the wide tables were extended coset by coset, 3 GB of other traffic between two reads of a tile).
    const unsigned bz = blockIdx.y;
    const fp *src = in + bz * in_batch_stride + (size_t)blockIdx.z * n;
    fp *dst = out + bz * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2;
    const ColsTables tb = cols_tables<LA, LB, LC>(aux, aux_ps, aux_ps_batch_stride, bz, log_c);
    const unsigned c = xcd_pair_tile(blockIdx.x) * L2 + l;

    fill_twiddles<LA, LB, LC>(tw, aux);
    fp a[A];
    cols_load_prescaled<LA, LB, LC>(a, src, tb.ps_row, log_c, t, c);
    reg_ntt_dif<LA, INV>(a); // step 1: rows r = r1 T + t; a[p] = Y[k1 = brev(p)]
    __syncthreads(); // tw[] ready
    const unsigned kh = t / Cn, r3 = t % Cn; // task h of this thread in step 2: k1 = kh + AH h, r3
    fp z[2][Bn];
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int p = 0; p < A; p++) {
            const unsigned k1 = cx_brev(p, LA);
            if ((int)(k1 / AH) == h) tile[((size_t)(k1 % AH) * T + t) * L2 + l] = (k1 == 0) ? a[p] : fp_mul(a[p], tw[k1 * t]);
        }
        __syncthreads();
#pragma unroll
        for (int r2 = 0; r2 < Bn; r2++) z[h][r2] = tile[((size_t)kh * T + r2 * Cn + r3) * L2 + l];
        __syncthreads(); // the half is rewritten
    }
    const unsigned k1s = t / Bn, k2 = t % Bn; // task h in step 3: k1 = k1s + AH h, k2
#pragma unroll
    for (int h = 0; h < 2; h++) {
        reg_ntt_dif<LB, INV>(z[h]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned j2 = cx_brev(p, LB);
            const fp v = (j2 == 0) ? z[h][p] : fp_mul(z[h][p], tw[(A * j2) * r3]);
            tile[((size_t)kh * T + j2 * Cn + (r3 ^ (j2 % Cn))) * L2 + l] = v;
        }
        __syncthreads();
        fp x[Cn];
#pragma unroll
        for (int q = 0; q < Cn; q++) x[q] = tile[((size_t)k1s * T + k2 * Cn + (q ^ (k2 % Cn))) * L2 + l];
        if (h == 0) __syncthreads(); // the half is rewritten by task 1
        reg_ntt_dif<LC, INV>(x);
        cols_store_task<LA, LB, LC>(x, (k1s + AH * h) + A * k2, c, log_c, tb, dst);
    }
}

// grid = (batch, R / L2, width), as k_ntt_rows_v4
template <int LA, int LB, int LC, bool INV>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), V5_ROWS_WAVES) void k_ntt_rows_v5(const fp *__restrict__ in, fp *__restrict__ out, unsigned log_n,
                                                                                    fp post_scale, int do_scale, size_t in_batch_stride,
                                                                                    size_t out_batch_stride, const fp *__restrict__ aux_tw) {
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, LOGM = G::LOGM, AH = A / 2;
    static_assert(G::J2 == 2 && G::J3 == 2 && Bn == AH && Cn == AH, "two tasks per thread and step, one per half");
    constexpr int TP = T + 4; // padded run of q per (j1, l), as in the v4 kernel
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                              // [A / 2][L2][TP]
    fp *tw = smem + (size_t)AH * L2 * TP;         // [M]
    const unsigned log_r = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const fp *src = in + blockIdx.x * in_batch_stride + (size_t)blockIdx.z * n;
    fp *dst = out + blockIdx.x * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned s1 = threadIdx.x % T, l1 = threadIdx.x / T; // step 1: s = c2 Cn + c3 fastest across lanes (coalesced row reads)
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2; // steps 2 and 3: l fastest across lanes (64-byte transposed stores)
    const unsigned k10 = xcd_pair_tile(blockIdx.y) * L2;
    fp a[A];
    const unsigned in_lane = (l1 << LOGM) + s1;
#pragma unroll
    for (int c1 = 0; c1 < A; c1++) a[c1] = mb_load(src + ((size_t)k10 << LOGM) + c1 * T, in_lane, in_lane + c1);
    fill_twiddles<LA, LB, LC>(tw, aux_tw); // after the tile loads: with the fill first hipcc spills 2 of the 80 VGPRs six waves per SIMD allow
    const unsigned jh = t / Cn, c3 = t % Cn;
    const unsigned j1s = t / Bn, j2s = t % Bn;
    reg_ntt_dif<LA, INV>(a); // step 1: columns c = c1 T + s
    __syncthreads(); // tw[] ready
    fp z[2][Bn];
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int p = 0; p < A; p++) {
            const unsigned j1 = cx_brev(p, LA);
            if ((int)(j1 / AH) == h) tile[((size_t)(j1 % AH) * L2 + l1) * TP + s1] = (j1 == 0) ? a[p] : fp_mul(a[p], tw[j1 * s1]);
        }
        __syncthreads();
#pragma unroll
        for (int c2 = 0; c2 < Bn; c2++) z[h][c2] = tile[((size_t)jh * L2 + l) * TP + c2 * Cn + c3];
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        reg_ntt_dif<LB, INV>(z[h]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned j2 = cx_brev(p, LB);
            const fp v = (j2 == 0) ? z[h][p] : fp_mul(z[h][p], tw[(A * j2) * c3]);
            tile[((size_t)jh * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))] = v;
        }
        __syncthreads();
        fp x[Cn];
#pragma unroll
        for (int q = 0; q < Cn; q++) x[q] = tile[((size_t)j1s * L2 + l) * TP + j2s * Cn + (q ^ (j2s % Cn))];
        if (h == 0) __syncthreads();
        reg_ntt_dif<LC, INV>(x);
        rows_store_task<LA, LB, LC>(x, (j1s + AH * h) + A * j2s, l, log_r, post_scale, do_scale, dst + k10);
    }
}

// k_ntt_rows_v5 for step columns, as k_ntt_rows_step_v4: the same steps with the tile formed by rows_load_step and no output scaling.
// Its own text: as a body shared with k_ntt_rows_v5 the register figures of that kernel stay but its code does not (26 instructions
// fewer, another schedule), and its dispatches of a proof measured 2 - 3 % longer (profiles/step_columns_ab.txt).
template <int LA, int LB, int LC>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), V5_ROWS_WAVES) void k_ntt_rows_step_v5(const fp *__restrict__ wtab, const fp *__restrict__ fac,
                                                                                         fp *__restrict__ out, unsigned log_n, unsigned log_t,
                                                                                         size_t out_batch_stride, const fp *__restrict__ aux_tw) {
    constexpr bool INV = false;
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, LOGM = G::LOGM, AH = A / 2;
    static_assert(G::J2 == 2 && G::J3 == 2 && Bn == AH && Cn == AH, "two tasks per thread and step, one per half");
    constexpr int TP = T + 4; // padded run of q per (j1, l), as in the v4 kernel
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                              // [A / 2][L2][TP]
    fp *tw = smem + (size_t)AH * L2 * TP;         // [M]
    const unsigned log_r = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const fp *src = wtab + blockIdx.x * n;
    fp *dst = out + blockIdx.x * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned s1 = threadIdx.x % T, l1 = threadIdx.x / T; // step 1: s = c2 Cn + c3 fastest across lanes (coalesced row reads)
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2; // steps 2 and 3: l fastest across lanes (64-byte transposed stores)
    const unsigned k10 = xcd_pair_tile(blockIdx.y) * L2;
    fp a[A];
    rows_load_step<LA, LB, LC>(a, src + ((size_t)k10 << LOGM), (l1 << LOGM) + s1, s1, fac + ((size_t)blockIdx.z << log_t), (1u << log_t) - 1);
    fill_twiddles<LA, LB, LC>(tw, aux_tw); // after the tile loads: with the fill first hipcc spills 2 of the 80 VGPRs six waves per SIMD allow
    const unsigned jh = t / Cn, c3 = t % Cn;
    const unsigned j1s = t / Bn, j2s = t % Bn;
    reg_ntt_dif<LA, INV>(a); // step 1: columns c = c1 T + s
    __syncthreads(); // tw[] ready
    fp z[2][Bn];
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int p = 0; p < A; p++) {
            const unsigned j1 = cx_brev(p, LA);
            if ((int)(j1 / AH) == h) tile[((size_t)(j1 % AH) * L2 + l1) * TP + s1] = (j1 == 0) ? a[p] : fp_mul(a[p], tw[j1 * s1]);
        }
        __syncthreads();
#pragma unroll
        for (int c2 = 0; c2 < Bn; c2++) z[h][c2] = tile[((size_t)jh * L2 + l) * TP + c2 * Cn + c3];
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        reg_ntt_dif<LB, INV>(z[h]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned j2 = cx_brev(p, LB);
            const fp v = (j2 == 0) ? z[h][p] : fp_mul(z[h][p], tw[(A * j2) * c3]);
            tile[((size_t)jh * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))] = v;
        }
        __syncthreads();
        fp x[Cn];
#pragma unroll
        for (int q = 0; q < Cn; q++) x[q] = tile[((size_t)j1s * L2 + l) * TP + j2s * Cn + (q ^ (j2s % Cn))];
        if (h == 0) __syncthreads();
        reg_ntt_dif<LC, INV>(x);
        rows_store_task<LA, LB, LC>(x, (j1s + AH * h) + A * j2s, l, log_r, 0, 0, dst + k10);
    }
}

// k_ntt_rows_step_v5 for two-level columns, as k_ntt_rows_step2_v4.
template <int LA, int LB, int LC>
__global__ __launch_bounds__((V4<LA, LB, LC>::NT), V5_ROWS_WAVES) void k_ntt_rows_step2_v5(const fp *__restrict__ wtab, const fp *__restrict__ wtab_r,
                                                                                          const fp *__restrict__ fac, fp *__restrict__ out, unsigned log_n,
                                                                                          unsigned log_t, size_t out_batch_stride,
                                                                                          const fp *__restrict__ aux_tw) {
    constexpr bool INV = false;
    using G = V4<LA, LB, LC>;
    constexpr int A = G::A, Bn = G::Bn, Cn = G::Cn, T = G::T, LOGM = G::LOGM, AH = A / 2;
    static_assert(G::J2 == 2 && G::J3 == 2 && Bn == AH && Cn == AH, "two tasks per thread and step, one per half");
    constexpr int TP = T + 4; // padded run of q per (j1, l), as in the v4 kernel
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    fp *tile = smem;                              // [A / 2][L2][TP]
    fp *tw = smem + (size_t)AH * L2 * TP;         // [M]
    const unsigned log_r = log_n - LOGM;
    const size_t n = (size_t)1 << log_n;
    const fp *src = wtab + blockIdx.x * n;
    const fp *src_r = wtab_r + blockIdx.x * n;
    const fp *fac_z = fac + ((size_t)blockIdx.z << (log_t + 1)); // A1 [T] | A2 [T]
    fp *dst = out + blockIdx.x * out_batch_stride + (size_t)blockIdx.z * n;
    const unsigned s1 = threadIdx.x % T, l1 = threadIdx.x / T; // step 1: s = c2 Cn + c3 fastest across lanes (coalesced row reads)
    const unsigned l = threadIdx.x % L2, t = threadIdx.x / L2; // steps 2 and 3: l fastest across lanes (64-byte transposed stores)
    const unsigned k10 = xcd_pair_tile(blockIdx.y) * L2;
    fp a[A];
    rows_load_step2<LA, LB, LC>(a, src + ((size_t)k10 << LOGM), src_r + ((size_t)k10 << LOGM), (l1 << LOGM) + s1, s1, fac_z, fac_z + ((size_t)1 << log_t),
                                (1u << log_t) - 1);
    fill_twiddles<LA, LB, LC>(tw, aux_tw); // after the tile loads: with the fill first hipcc spills 2 of the 80 VGPRs six waves per SIMD allow
    const unsigned jh = t / Cn, c3 = t % Cn;
    const unsigned j1s = t / Bn, j2s = t % Bn;
    reg_ntt_dif<LA, INV>(a); // step 1: columns c = c1 T + s
    __syncthreads(); // tw[] ready
    fp z[2][Bn];
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int p = 0; p < A; p++) {
            const unsigned j1 = cx_brev(p, LA);
            if ((int)(j1 / AH) == h) tile[((size_t)(j1 % AH) * L2 + l1) * TP + s1] = (j1 == 0) ? a[p] : fp_mul(a[p], tw[j1 * s1]);
        }
        __syncthreads();
#pragma unroll
        for (int c2 = 0; c2 < Bn; c2++) z[h][c2] = tile[((size_t)jh * L2 + l) * TP + c2 * Cn + c3];
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        reg_ntt_dif<LB, INV>(z[h]);
#pragma unroll
        for (int p = 0; p < Bn; p++) {
            const unsigned j2 = cx_brev(p, LB);
            const fp v = (j2 == 0) ? z[h][p] : fp_mul(z[h][p], tw[(A * j2) * c3]);
            tile[((size_t)jh * L2 + l) * TP + j2 * Cn + (c3 ^ (j2 % Cn))] = v;
        }
        __syncthreads();
        fp x[Cn];
#pragma unroll
        for (int q = 0; q < Cn; q++) x[q] = tile[((size_t)j1s * L2 + l) * TP + j2s * Cn + (q ^ (j2s % Cn))];
        if (h == 0) __syncthreads();
        reg_ntt_dif<LC, INV>(x);
        rows_store_task<LA, LB, LC>(x, (j1s + AH * h) + A * j2s, l, log_r, 0, 0, dst + k10);
    }
}

// The sizes served by the three-step kernels -- the ONE list: both passes of n = 2^(2 LOGM) points split LOGM = LA + LB + LC, with
// whole-tile (v4) or half-tile (v5) exchanges.  ntt_three_step_shape and ntt_columns both read it.
template <int LA_, int LB_, int LC_, bool HALF_TILE_>
struct ThreeStep { static constexpr int LA = LA_, LB = LB_, LC = LC_; static constexpr bool HALF_TILE = HALF_TILE_; };
template <class F>
bool three_step_size(unsigned log_n, F &&f) {
    switch (log_n) {
    case 20: f(ThreeStep<4, 3, 3, true>{}); return true;
    case 18: f(ThreeStep<3, 3, 3, false>{}); return true;
    case 16: f(ThreeStep<3, 3, 2, false>{}); return true;
    default: return false;
    }
}

// Both passes of one three-step size.  The dense tables are not optional: get_plan / get_coset_table (capi.hip) build them for
// exactly the sizes of three_step_size, and a caller that comes without them is refused -- there is no slower table-less path.
// `step` (forward only): instead of the pair, either the column pass alone (step->wtab == nullptr: a.scratch receives it -- how the
// step-column tables are built) or the row pass of step columns alone (reads step->wtab and step->fac, no scratch; with step->wtab_r
// the row pass of two-level columns, fac holding both sets of factors)
struct StepPass { const fp *wtab, *fac; unsigned log_t; const fp *wtab_r = nullptr; };
template <class S, bool INV>
hipError_t launch_three_step(const NttArgs &a, hipStream_t stream, const StepPass *step = nullptr) {
    using G = V4<S::LA, S::LB, S::LC>;
    if (!a.aux || (a.prescale && !a.aux_ps) || (step && INV)) return hipErrorInvalidValue;
    const bool do_cols = !step || !step->wtab, do_rows = !step;
    constexpr int HALVES = S::HALF_TILE ? 2 : 1; // the tile in LDS holds all or half of the 2^LA k1 classes
    const size_t lds_cols = ((size_t)G::M / HALVES * L2 + G::M) * sizeof(fp);
    const size_t lds_rows = ((size_t)G::A / HALVES * L2 * (G::T + 4) + G::M) * sizeof(fp);
    const dim3 grid_cols((unsigned)G::M / L2, a.batch, a.width), grid_rows(a.batch, (unsigned)G::M / L2, a.width);
    const fp *aux_ps = a.prescale ? a.aux_ps : nullptr;
    hipError_t e;
    if constexpr (S::HALF_TILE) {
        const auto k_cols = k_ntt_cols_v5<S::LA, S::LB, S::LC, INV>;
        const auto k_rows = k_ntt_rows_v5<S::LA, S::LB, S::LC, INV>;
        if ((e = hipFuncSetAttribute((const void *)k_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)) != hipSuccess) return e;
        if ((e = hipFuncSetAttribute((const void *)k_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cols)) != hipSuccess) return e;
        if (do_cols)
            hipLaunchKernelGGL(k_cols, grid_cols, dim3(G::NT), lds_cols, stream, a.in, a.scratch, a.log_n, a.in_batch_stride, a.scratch_batch_stride, a.aux,
                               aux_ps, a.aux_ps_batch_stride);
        if (do_rows)
            hipLaunchKernelGGL(k_rows, grid_rows, dim3(G::NT), lds_rows, stream, (const fp *)a.scratch, a.out, a.log_n, a.post_scale, a.do_scale ? 1 : 0,
                               a.scratch_batch_stride, a.out_batch_stride, a.aux + G::M);
        if constexpr (!INV) {
            if (step && step->wtab) {
                const auto k_step = k_ntt_rows_step_v5<S::LA, S::LB, S::LC>;
                const auto k_step2 = k_ntt_rows_step2_v5<S::LA, S::LB, S::LC>;
                if ((e = hipFuncSetAttribute((const void *)k_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)) != hipSuccess) return e;
                if ((e = hipFuncSetAttribute((const void *)k_step2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)) != hipSuccess) return e;
                if (step->wtab_r)
                    hipLaunchKernelGGL(k_step2, grid_rows, dim3(G::NT), lds_rows, stream, step->wtab, step->wtab_r, step->fac, a.out, a.log_n, step->log_t,
                                       a.out_batch_stride, a.aux + G::M);
                else
                    hipLaunchKernelGGL(k_step, grid_rows, dim3(G::NT), lds_rows, stream, step->wtab, step->fac, a.out, a.log_n, step->log_t,
                                       a.out_batch_stride, a.aux + G::M);
            }
        }
    } else {
        const auto k_cols = k_ntt_cols_v4<S::LA, S::LB, S::LC, INV>;
        const auto k_rows = k_ntt_rows_v4<S::LA, S::LB, S::LC, INV>;
        if ((e = hipFuncSetAttribute((const void *)k_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)) != hipSuccess) return e;
        if ((e = hipFuncSetAttribute((const void *)k_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cols)) != hipSuccess) return e;
        if (do_cols)
            hipLaunchKernelGGL(k_cols, grid_cols, dim3(G::NT), lds_cols, stream, a.in, a.scratch, a.log_n, a.w, a.prescale, a.in_batch_stride,
                               a.scratch_batch_stride, a.prescale_batch_stride, a.aux, aux_ps, a.aux_ps_batch_stride);
        if (do_rows)
            hipLaunchKernelGGL(k_rows, grid_rows, dim3(G::NT), lds_rows, stream, (const fp *)a.scratch, a.out, a.log_n, a.w, a.post_scale, a.do_scale ? 1 : 0,
                               a.scratch_batch_stride, a.out_batch_stride, a.aux + G::M);
        if constexpr (!INV) {
            if (step && step->wtab) {
                const auto k_step = k_ntt_rows_step_v4<S::LA, S::LB, S::LC>;
                const auto k_step2 = k_ntt_rows_step2_v4<S::LA, S::LB, S::LC>;
                if ((e = hipFuncSetAttribute((const void *)k_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)) != hipSuccess) return e;
                if ((e = hipFuncSetAttribute((const void *)k_step2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)) != hipSuccess) return e;
                if (step->wtab_r)
                    hipLaunchKernelGGL(k_step2, grid_rows, dim3(G::NT), lds_rows, stream, step->wtab, step->wtab_r, step->fac, a.out, a.log_n, step->log_t,
                                       a.out_batch_stride, a.aux + G::M);
                else
                    hipLaunchKernelGGL(k_step, grid_rows, dim3(G::NT), lds_rows, stream, step->wtab, step->fac, a.out, a.log_n, step->log_t,
                                       a.out_batch_stride, a.aux + G::M);
            }
        }
    }
    return hipGetLastError();
}

// table[e] = base^e for e < n; each thread produces CHUNK consecutive powers
constexpr int CHUNK = 16;
__global__ void k_power_table(fp *table, size_t n, fp base) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t e0 = t * CHUNK;
    if (e0 >= n) return;
    fp x = fp_pow(base, e0);
    for (int i = 0; i < CHUNK && e0 + i < n; i++) { table[e0 + i] = x; x = fp_mul(x, base); }
}

// The generic pass pair with L columns / rows per workgroup
template <int L>
hipError_t launch(const NttArgs &a, hipStream_t stream) {
    const unsigned log_r = (a.log_n + 1) / 2, log_c = a.log_n - log_r;
    const unsigned R = 1u << log_r, C = 1u << log_c;
    const size_t lds_a = ((size_t)R * L + R / 2) * sizeof(fp), lds_b = ((size_t)C * L + C / 2) * sizeof(fp);
    hipError_t e;
    if ((e = hipFuncSetAttribute((const void *)k_ntt_cols<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a)) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute((const void *)k_ntt_rows<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ntt_cols<L>, dim3(C / L, a.width, a.batch), dim3(NT), lds_a, stream, a.in, a.scratch, a.log_n, log_r, a.w, a.prescale,
                       a.in_batch_stride, a.scratch_batch_stride, a.prescale_batch_stride);
    hipLaunchKernelGGL(k_ntt_rows<L>, dim3(R / L, a.width, a.batch), dim3(NT), lds_b, stream, (const fp *)a.scratch, a.out, a.log_n, log_r, a.w,
                       a.post_scale, a.do_scale ? 1 : 0, a.scratch_batch_stride, a.out_batch_stride);
    return hipGetLastError();
}

} // namespace

// Composition-polynomial column split: h holds the N = b*n coefficients of H(g y) in y; column i of out gets
// H_i[q] = h[b*q + i] * g^-(b*q + i)  (coefficients of H in x, H(x) = sum_i x^i H_i(x^b)).  One thread per q.
__global__ void k_split_columns(const fp *__restrict__ h, fp *__restrict__ out, size_t n, unsigned log_b, fp ginv) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= n) return;
    const unsigned b = 1u << log_b;
    fp s = fp_pow(ginv, (uint64_t)q << log_b);
    for (unsigned i = 0; i < b; i++) {
        out[(size_t)i * n + q] = fp_mul(h[((size_t)q << log_b) + i], s);
        s = fp_mul(s, ginv);
    }
}
hipError_t split_columns(const fp *d_h, fp *d_out, unsigned log_n, unsigned log_b, fp ginv, hipStream_t stream) {
    const size_t n = (size_t)1 << log_n;
    hipLaunchKernelGGL(k_split_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_h, d_out, n, log_b, ginv);
    return hipGetLastError();
}
// natural[b*j + k] = coset_major[k*n + j]
__global__ void k_interleave_cosets(const fp *__restrict__ in, fp *__restrict__ out, size_t n, unsigned log_b) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (n << log_b)) return;
    const size_t k = i & ((1u << log_b) - 1), j = i >> log_b;
    out[i] = in[k * n + j];
}
hipError_t interleave_cosets(const fp *d_in, fp *d_out, unsigned log_n, unsigned log_b, hipStream_t stream) {
    const size_t N = (size_t)1 << (log_n + log_b);
    hipLaunchKernelGGL(k_interleave_cosets, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, d_in, d_out, (size_t)1 << log_n, log_b);
    return hipGetLastError();
}

// one thread per q: the B values of row q across the cosets, twisted and put through a B-point inverse DFT (B <= 8: B^2 products)
template <int LOGB>
__global__ __launch_bounds__(256) void k_coset_combine(const fp *__restrict__ in, fp *__restrict__ out, size_t n, const fp *__restrict__ winv, fp b_inv) {
    constexpr int B = 1 << LOGB;
    const size_t q = blockIdx.x * (size_t)256 + threadIdx.x;
    if (q >= n) return;
    in += (size_t)blockIdx.y * B * n; // grid.y = table
    out += (size_t)blockIdx.y * B * n;
    fp v[B], wb[B];
#pragma unroll
    for (int k = 0; k < B; k++) {
        wb[k] = winv[(size_t)k * n];                                   // w_B^-k
        const fp x = in[(size_t)k * n + q];
        v[k] = k == 0 ? fp_mul(x, b_inv) : fp_mul(fp_mul(x, b_inv), winv[(size_t)k * q]); // (1 / B) w_N^(-k q) B_k[q]
    }
#pragma unroll
    for (int i = 0; i < B; i++) {
        Acc128 a = acc_zero();
#pragma unroll
        for (int k = 0; k < B; k++) {
            acc_mad(a, v[k], wb[(k * i) & (B - 1)]);
            if (k == 6) acc_fold(a);
        }
        acc_fold(a);
        out[(size_t)i * n + q] = acc_reduce(a);
    }
}
// (kc0, nkc): only even cosets [kc0, kc0 + nkc) of `in` are present, the others count as zero (one rank's share of a sharded proof:
// the map is linear, the ranks' outputs add up)
__global__ __launch_bounds__(256) void k_coset_even_to_odd(const fp *__restrict__ in, fp *__restrict__ out, size_t n, unsigned tables,
                                                           const fp *__restrict__ winv4n, const fp *__restrict__ w8n, fp quarter, unsigned kc0, unsigned nkc) {
    const size_t q = blockIdx.x * (size_t)256 + threadIdx.x;
    if (q >= n) return;
    const unsigned tb = blockIdx.y;
    fp v[4], w4[4], w8[8], a[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        w4[k] = winv4n[(size_t)k * n]; // w_4^-k
        const fp x = ((unsigned)k - kc0 < nkc) ? fp_mul(in[((size_t)tb * 4 + k) * n + q], quarter) : 0;
        v[k] = k == 0 ? x : fp_mul(x, winv4n[(size_t)k * q]);
    }
#pragma unroll
    for (int e = 0; e < 8; e++) w8[e] = w8n[(size_t)e * n]; // w_8^e
#pragma unroll
    for (int i = 0; i < 4; i++) { // coefficient a_{q + n i}
        fp s = v[0];
#pragma unroll
        for (int k = 1; k < 4; k++) s = fp_add(s, fp_mul(v[k], w4[(k * i) & 3]));
        a[i] = s;
    }
#pragma unroll
    for (int kc = 0; kc < 4; kc++) {
        const int k = 2 * kc + 1;
        fp s = a[0];
#pragma unroll
        for (int i = 1; i < 4; i++) s = fp_add(s, fp_mul(a[i], w8[(k * i) & 7]));
        out[((size_t)kc * tables + tb) * n + q] = s;
    }
}
hipError_t coset_even_to_odd(const fp *d_b, fp *d_out, unsigned log_n, unsigned tables, const fp *d_winv_4n, const fp *d_w_8n, fp quarter,
                             hipStream_t stream, unsigned kc0, unsigned nkc) {
    const size_t n = (size_t)1 << log_n;
    hipLaunchKernelGGL(k_coset_even_to_odd, dim3((unsigned)((n + 255) / 256), tables), dim3(256), 0, stream, d_b, d_out, n, tables, d_winv_4n, d_w_8n, quarter,
                       kc0, nkc);
    return hipGetLastError();
}
// grid = (n / 256, families, sets): a thread owns output index q' of one family.  Per term the four interpolants are read at
// (q' - r) mod n (shifted, still coalesced) and taken to the odd cosets as in k_coset_even_to_odd; the term's constant (the wrapped
// entries: times y^n) and the sum over the family follow in registers.
__global__ __launch_bounds__(256) void k_coset_even_to_odd_merged(const fp *__restrict__ in, fp *__restrict__ out, size_t n, CosetMergeDesc d,
                                                                  const fp *__restrict__ winv4n, const fp *__restrict__ w8n, fp quarter,
                                                                  fp *__restrict__ raw) {
    const size_t q = blockIdx.x * (size_t)256 + threadIdx.x;
    if (q >= n) return;
    const unsigned fam = blockIdx.y, set = blockIdx.z;
    fp w4[4], w8[8], acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++) w4[k] = winv4n[(size_t)k * n]; // w_4^-k
#pragma unroll
    for (int e = 0; e < 8; e++) w8[e] = w8n[(size_t)e * n]; // w_8^e
    const unsigned terms = d.terms[fam];
#pragma unroll 1
    for (unsigned t = 0; t < terms; t++) {
        const CosetMergeTerm &tm = d.term[fam][t];
        const size_t qs = (q - tm.r) & (n - 1);
        const bool wrapped = q < tm.r;
        const fp *tab = in + ((size_t)set * d.tables_per_set + tm.table) * 4 * n + qs;
        fp v[4], a[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const fp x = fp_mul(tab[(size_t)k * n], quarter);
            v[k] = k == 0 ? x : fp_mul(x, winv4n[(size_t)k * qs]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { // coefficient a_{qs + n i}
            fp s = v[0];
#pragma unroll
            for (int k = 1; k < 4; k++) s = fp_add(s, fp_mul(v[k], w4[(k * i) & 3]));
            a[i] = s;
        }
#pragma unroll
        for (int kc = 0; kc < 4; kc++) {
            const int k = 2 * kc + 1;
            fp s = a[0];
#pragma unroll
            for (int i = 1; i < 4; i++) s = fp_add(s, fp_mul(a[i], w8[(k * i) & 7]));
            if (kc == 0 && raw && (int)fam == d.raw_family) raw[((size_t)set * terms + t) * n + qs] = fp_mul(s, w8n[qs]);
            acc[kc] = fp_add(acc[kc], fp_mul(s, tm.c[kc][wrapped ? 1 : 0]));
        }
    }
#pragma unroll
    for (int kc = 0; kc < 4; kc++) out[(((size_t)kc * gridDim.z + set) * d.families + fam) * n + q] = acc[kc];
}
CosetMergeTerm coset_merge_term(unsigned table, uint64_t e, unsigned log_n, uint64_t base, unsigned k0) {
    CosetMergeTerm t{};
    const uint64_t n = 1ull << log_n, dq = e >> log_n, w8 = host::root_of_unity(3);
    t.table = table;
    t.r = (uint32_t)(e & (n - 1));
    const uint64_t be = host::pow(base, e);
    for (unsigned i = 0; i < 4; i++) {
        const uint64_t k = k0 + 2 * i;
        t.c[i][0] = host::mul(be, host::pow(w8, (k * (dq & 7)) & 7));
        t.c[i][1] = host::mul(t.c[i][0], host::pow(w8, k & 7));
    }
    return t;
}
hipError_t coset_even_to_odd_merged(const fp *d_b, fp *d_out, unsigned log_n, unsigned sets, const CosetMergeDesc &desc, const fp *d_winv_4n,
                                    const fp *d_w_8n, fp quarter, fp *d_raw, hipStream_t stream) {
    const size_t n = (size_t)1 << log_n;
    if (desc.families == 0 || desc.families > (unsigned)COSET_MERGE_MAX_FAMILIES || sets == 0) return hipErrorInvalidValue;
    for (unsigned f = 0; f < desc.families; f++) {
        if (desc.terms[f] == 0 || desc.terms[f] > (unsigned)COSET_MERGE_MAX_TERMS) return hipErrorInvalidValue;
        for (unsigned t = 0; t < desc.terms[f]; t++)
            if (desc.term[f][t].table >= desc.tables_per_set || desc.term[f][t].r >= n) return hipErrorInvalidValue;
    }
    if (desc.raw_family >= (int)desc.families) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_coset_even_to_odd_merged, dim3((unsigned)((n + 255) / 256), desc.families, sets), dim3(256), 0, stream, d_b, d_out, n, desc,
                       d_winv_4n, d_w_8n, quarter, d_raw);
    return hipGetLastError();
}
hipError_t coset_combine(const fp *d_b, fp *d_h, unsigned log_n, unsigned log_b, const fp *d_winv_N, fp b_inv, hipStream_t stream, unsigned tables) {
    const size_t n = (size_t)1 << log_n;
    const dim3 grid((unsigned)((n + 255) / 256), tables), block(256);
    if (log_b == 1) hipLaunchKernelGGL(k_coset_combine<1>, grid, block, 0, stream, d_b, d_h, n, d_winv_N, b_inv);
    else if (log_b == 2) hipLaunchKernelGGL(k_coset_combine<2>, grid, block, 0, stream, d_b, d_h, n, d_winv_N, b_inv);
    else if (log_b == 3) hipLaunchKernelGGL(k_coset_combine<3>, grid, block, 0, stream, d_b, d_h, n, d_winv_N, b_inv);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- compact tables of the three-step kernels ------------------------------------------------------------------------
// The twiddles of a sub-transform, the row part of a coset's prescale and the output factors of the column pass are strided or
// scattered entries of the n-entry tables (w[e << log_c], s[r << log_c], w[kb c]): 8 useful bytes per 64-byte sector and, for the
// output factors, one sector per lane.  Gathered once per table into dense arrays, a workgroup reads them as a handful of
// contiguous lines: 2.3 k instead of 5 k sector requests per column-pass workgroup.
bool ntt_three_step_shape(unsigned log_n, NttThreeStepShape *s) {
    return three_step_size(log_n, [s](auto split) {
        using S = decltype(split);
        *s = {S::LA + S::LB + S::LC, S::LA + S::LB + S::LC, S::LA + S::LB}; // both passes over 2^LOGM points; kb = k1 + 2^LA k2
    });
}
namespace {
// plan block: [R] w^(e C) | [C] w^(e R) | [C] w^(KB c) | [KB][C] w^(kb c)
__global__ void k_aux_plan(fp *aux, const fp *__restrict__ w, unsigned log_r, unsigned log_c, unsigned log_kb) {
    const size_t R = (size_t)1 << log_r, C = (size_t)1 << log_c, total = R + 2 * C + (C << log_kb);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        fp v;
        if (i < R) v = w[i << log_c];
        else if (i < R + C) v = w[(i - R) << log_r];
        else if (i < R + 2 * C) v = w[(i - R - C) << log_kb];
        else { const size_t q = i - R - 2 * C, kb = q >> log_c, c = q & (C - 1); v = w[kb * c]; }
        aux[i] = v;
    }
}
// coset block: [R] s^(r C) | [KB][C] w^(kb c) s^c
__global__ void k_aux_coset(fp *aux, const fp *__restrict__ w, const fp *__restrict__ s, unsigned log_r, unsigned log_c, unsigned log_kb) {
    const size_t R = (size_t)1 << log_r, C = (size_t)1 << log_c, total = R + (C << log_kb);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        fp v;
        if (i < R) v = s[i << log_c];
        else { const size_t q = i - R, kb = q >> log_c, c = q & (C - 1); v = fp_mul(w[kb * c], s[c]); }
        aux[i] = v;
    }
}
} // namespace
size_t ntt_aux_plan_words(const NttThreeStepShape &s) { return ((size_t)1 << s.log_r) + ((size_t)2 << s.log_c) + ((size_t)1 << (s.log_c + s.log_kb)); }
size_t ntt_aux_coset_words(const NttThreeStepShape &s) { return ((size_t)1 << s.log_r) + ((size_t)1 << (s.log_c + s.log_kb)); }
hipError_t ntt_build_aux_plan(fp *d_aux, const fp *d_w, const NttThreeStepShape &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_aux_plan, dim3(256), dim3(256), 0, stream, d_aux, d_w, s.log_r, s.log_c, s.log_kb);
    return hipGetLastError();
}
hipError_t ntt_build_aux_coset(fp *d_aux, const fp *d_w, const fp *d_s, const NttThreeStepShape &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_aux_coset, dim3(256), dim3(256), 0, stream, d_aux, d_w, d_s, s.log_r, s.log_c, s.log_kb);
    return hipGetLastError();
}

// ---- step columns ----------------------------------------------------------------------------------------------------
// A column that is constant over blocks of B = 2^log_block rows, f[i] = g[i >> log_block] (T = n / B block values), has the
// interpolant  c_k = A[k mod T] D[k]:  with z = w_n^B (a T-th root of unity) and G^[j] = sum_t g[t] z^(-t j),
//   A[0] = G^[0] / T,  A[j] = G^[j] (z^(-j) - 1) / n;   D[0] = 1,  D[k] = 0 for T | k, k != 0,  D[k] = 1 / (w_n^(-k) - 1) otherwise
// (c_k = (1/n) sum_t g[t] z^(-t k) sum_{r<B} w_n^(-r k): the inner sum is B at k = 0 and the geometric quotient elsewhere).  D depends
// on (n, B) alone.  The column pass of the three-step transform works on every column class c = k mod C by itself and linearly, so
// for T | C it sends c_k to A[c mod T] W[k1][c], W = the column pass of D: a table per coset, built once.  A step column then costs a
// T-point transform, the pointwise coefficient table and, per coset, the row pass alone with W A formed at its loads.
//
// Two-level columns: f[t B + r] = u[t] for r < R, v[t] for r >= R (0 < R < B) is the step column of v plus (u - v) on the first R
// rows of every block, so with A1 = the factors A of v and Delta^[j] = sum_t (u - v)[t] z^(-t j)
//   c_k = A1[k mod T] D[k] + A2[k mod T] D_R[k],   A2[j] = Delta^[j] / n,   D_R[k] = sum_{r<R} w_n^(-r k):
//   D_R[0] = R,  D_R[k] = (w_n^(-R k) - 1) / (w_n^(-k) - 1) otherwise
// D_R depends on (n, R) alone, its column pass W_R is a second table per coset, and the row pass takes W A1 + W_R A2 at its loads.
bool ntt_step_shape(unsigned log_n, unsigned log_block) {
    NttThreeStepShape s;
    return log_block < log_n && ntt_three_step_shape(log_n, &s) && log_n - log_block <= s.log_c;
}
namespace {
__global__ __launch_bounds__(256) void k_step_d(fp *__restrict__ d, const fp *__restrict__ winv, size_t n, unsigned log_t) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= n) return;
    d[k] = k == 0 ? FP_ONE : (k & (((size_t)1 << log_t) - 1)) == 0 ? 0 : fp_inv(fp_sub(winv[k], FP_ONE));
}
// D_R [n] of the two-level columns: r_mont = R in Montgomery form; w_n^(-R k) is winv[R k mod n]
__global__ __launch_bounds__(256) void k_step_dr(fp *__restrict__ d, const fp *__restrict__ winv, size_t n, unsigned split, fp r_mont) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= n) return;
    d[k] = k == 0 ? r_mont : fp_mul(fp_sub(winv[(k * split) & (n - 1)], FP_ONE), fp_inv(fp_sub(winv[k], FP_ONE)));
}
// grid = columns: one workgroup gathers the T block values of its column (the first row of every block), transforms them in LDS and
// writes the T factors A
__global__ __launch_bounds__(NT) void k_step_factors(const fp *__restrict__ evals, fp *__restrict__ fac, unsigned log_n, unsigned log_t,
                                                     const fp *__restrict__ winv, fp n_inv, fp t_inv) {
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    const unsigned T = 1u << log_t, log_block = log_n - log_t;
    fp *tile = smem, *tw = smem + T;
    const fp *col = evals + ((size_t)blockIdx.x << log_n);
    for (unsigned t = threadIdx.x; t < T; t += NT) tile[t] = col[(size_t)t << log_block];
    for (unsigned e = threadIdx.x; e < T / 2; e += NT) tw[e] = winv[(size_t)e << log_block];
    __syncthreads();
    lds_ntt_dif<1>(tile, log_t, tw);
    for (unsigned j = threadIdx.x; j < T; j += NT) {
        const fp g = tile[bitrev(j, log_t)];
        fac[((size_t)blockIdx.x << log_t) + j] = j == 0 ? fp_mul(g, t_inv) : fp_mul(fp_mul(g, n_inv), fp_sub(winv[(size_t)j << log_block], FP_ONE));
    }
}
// The same for a two-level column: rows `split` (v) and 0 (u) of every block; fac [column][2][T] = A1 (of v) | A2 (of u - v)
__global__ __launch_bounds__(NT) void k_step2_factors(const fp *__restrict__ evals, fp *__restrict__ fac, unsigned log_n, unsigned log_t, unsigned split,
                                                      const fp *__restrict__ winv, fp n_inv, fp t_inv) {
    extern __shared__ __attribute__((aligned(16))) fp smem[];
    const unsigned T = 1u << log_t, log_block = log_n - log_t;
    fp *tile = smem, *tile_d = smem + T, *tw = smem + 2 * T;
    const fp *col = evals + ((size_t)blockIdx.x << log_n);
    for (unsigned t = threadIdx.x; t < T; t += NT) {
        const fp v = col[((size_t)t << log_block) + split];
        tile[t] = v;
        tile_d[t] = fp_sub(col[(size_t)t << log_block], v);
    }
    for (unsigned e = threadIdx.x; e < T / 2; e += NT) tw[e] = winv[(size_t)e << log_block];
    __syncthreads();
    lds_ntt_dif<1>(tile, log_t, tw);
    lds_ntt_dif<1>(tile_d, log_t, tw);
    fp *out = fac + ((size_t)blockIdx.x << (log_t + 1));
    for (unsigned j = threadIdx.x; j < T; j += NT) {
        const fp g = tile[bitrev(j, log_t)];
        out[j] = j == 0 ? fp_mul(g, t_inv) : fp_mul(fp_mul(g, n_inv), fp_sub(winv[(size_t)j << log_block], FP_ONE));
        out[T + j] = fp_mul(tile_d[bitrev(j, log_t)], n_inv);
    }
}
// grid = (n / 256, columns)
__global__ __launch_bounds__(256) void k_step2_coeffs(const fp *__restrict__ fac, const fp *__restrict__ d, const fp *__restrict__ dr, fp *__restrict__ coeffs,
                                                      unsigned log_n, unsigned log_t) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x, j = k & (((size_t)1 << log_t) - 1);
    const fp *f = fac + ((size_t)blockIdx.y << (log_t + 1));
    coeffs[((size_t)blockIdx.y << log_n) + k] = fp_add(fp_mul(f[j], d[k]), fp_mul(f[((size_t)1 << log_t) + j], dr[k]));
}
// grid = (n / 256, columns)
__global__ __launch_bounds__(256) void k_step_coeffs(const fp *__restrict__ fac, const fp *__restrict__ d, fp *__restrict__ coeffs, unsigned log_n,
                                                     unsigned log_t) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    coeffs[((size_t)blockIdx.y << log_n) + k] = fp_mul(fac[((size_t)blockIdx.y << log_t) + (k & (((size_t)1 << log_t) - 1))], d[k]);
}
} // namespace
hipError_t ntt_step_build_tables(uint64_t *d_d, unsigned log_block, unsigned split, const uint64_t *d_winv, const NttArgs &a, hipStream_t stream) {
    if (!ntt_step_shape(a.log_n, log_block) || a.inverse || a.width != 1 || a.in != d_d || split >= (1u << log_block)) return hipErrorInvalidValue;
    const size_t n = (size_t)1 << a.log_n;
    if (split == 0) hipLaunchKernelGGL(k_step_d, dim3((unsigned)(n / 256)), dim3(256), 0, stream, d_d, d_winv, n, a.log_n - log_block);
    else hipLaunchKernelGGL(k_step_dr, dim3((unsigned)(n / 256)), dim3(256), 0, stream, d_d, d_winv, n, split, host::from_u64(split));
    const StepPass columns_only{nullptr, nullptr, 0};
    hipError_t e = hipErrorInvalidValue;
    three_step_size(a.log_n, [&](auto split) { e = launch_three_step<decltype(split), false>(a, stream, &columns_only); });
    return e;
}
hipError_t ntt_step_coefficients(const uint64_t *d_evals, uint64_t *d_fac, uint64_t *d_coeffs, const uint64_t *d_d, unsigned ncols, unsigned log_n,
                                 unsigned log_block, const uint64_t *d_winv, uint64_t n_inv, hipStream_t stream) {
    if (!ntt_step_shape(log_n, log_block) || ncols == 0 || ncols > 65535) return hipErrorInvalidValue;
    const unsigned log_t = log_n - log_block;
    const uint64_t t_inv = host::inv(host::from_u64((uint64_t)1 << log_t));
    hipLaunchKernelGGL(k_step_factors, dim3(ncols), dim3(NT), (size_t)3 * 8 << (log_t - 1), stream, d_evals, d_fac, log_n, log_t, d_winv, n_inv, t_inv);
    hipLaunchKernelGGL(k_step_coeffs, dim3((unsigned)(((size_t)1 << log_n) / 256), ncols), dim3(256), 0, stream, (const fp *)d_fac, d_d, d_coeffs, log_n,
                       log_t);
    return hipGetLastError();
}
hipError_t ntt_step2_coefficients(const uint64_t *d_evals, uint64_t *d_fac, uint64_t *d_coeffs, const uint64_t *d_d, const uint64_t *d_dr, unsigned ncols,
                                  unsigned log_n, unsigned log_block, unsigned split, const uint64_t *d_winv, uint64_t n_inv, hipStream_t stream) {
    if (!ntt_step_shape(log_n, log_block) || ncols == 0 || ncols > 65535 || split == 0 || split >= (1u << log_block)) return hipErrorInvalidValue;
    const unsigned log_t = log_n - log_block;
    const uint64_t t_inv = host::inv(host::from_u64((uint64_t)1 << log_t));
    hipLaunchKernelGGL(k_step2_factors, dim3(ncols), dim3(NT), (size_t)5 * 8 << (log_t - 1), stream, d_evals, d_fac, log_n, log_t, split, d_winv, n_inv, t_inv);
    hipLaunchKernelGGL(k_step2_coeffs, dim3((unsigned)(((size_t)1 << log_n) / 256), ncols), dim3(256), 0, stream, (const fp *)d_fac, d_d, d_dr, d_coeffs,
                       log_n, log_t);
    return hipGetLastError();
}
hipError_t ntt_step_rows(const NttArgs &a, const uint64_t *d_wtab, const uint64_t *d_wtab_r, const uint64_t *d_fac, unsigned log_block, hipStream_t stream) {
    if (!ntt_step_shape(a.log_n, log_block) || a.inverse || !d_wtab || !d_fac) return hipErrorInvalidValue;
    const StepPass rows{d_wtab, d_fac, a.log_n - log_block, d_wtab_r};
    hipError_t e = hipErrorInvalidValue;
    three_step_size(a.log_n, [&](auto split) { e = launch_three_step<decltype(split), false>(a, stream, &rows); });
    return e;
}

hipError_t ntt_power_table(fp *d_table, size_t n, fp base, hipStream_t stream) {
    const size_t threads = (n + CHUNK - 1) / CHUNK;
    hipLaunchKernelGGL(k_power_table, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, d_table, n, base);
    return hipGetLastError();
}

hipError_t ntt_columns(const NttArgs &a, hipStream_t stream) {
    if (a.log_n < NTT_MIN_LOG_N || a.log_n > NTT_MAX_LOG_N) return hipErrorInvalidValue;
    // register kernels for the product sizes; `inverse` selects the compile-time small twiddles
    hipError_t e = hipSuccess;
    if (three_step_size(a.log_n, [&](auto split) {
            using S = decltype(split);
            e = a.inverse ? launch_three_step<S, true>(a, stream) : launch_three_step<S, false>(a, stream);
        }))
        return e;
    // every other size: L = 8 keeps global segments at 64 bytes; sub-transforms above 2^11 points need the narrower tile to fit LDS
    return (a.log_n + 1) / 2 <= 11 ? launch<8>(a, stream) : launch<4>(a, stream);
}

} // namespace cs
