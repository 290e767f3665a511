// Trace validation (cstark_air_validate_trace): the transition constraints of the five AIRs on the TRACE domain, the
// boundary lists, and the gather of one frame for the free-standing-frame evaluator.  A translation unit of its own, so that the code
// object of constraints.hip -- the proof's constraint stage -- is what it was before these kernels existed; the constraint bodies are
// the templates of constraint_bodies.cuh, shared with constraints.hip.
#include "constraint_bodies.cuh"

namespace cs {

// Trace validation: the transition constraints on the TRACE domain, what the reference's debug build does in
// trace.validate(&air).  The bodies are the templates of constraint_bodies.cuh behind one more accumulator: the slot sums of a wave's 64 consecutive
// frames stay in LDS, tile[slot][lane]; a lane touches only its own column (8-byte accesses, no bank conflicts, no barrier).  A slot is
// violated when its SUM over all (flag, value) contributions is non-zero, so the zero test comes after every contribution.
// Frame r = (row r, row r + 1), r < n - 1; the periodic values are the raw columns at r mod cycle_len.  Per cycle r / cycle_len the
// result is min over its violated frames of (r mod cycle_len) * NC + lowest violated slot, by atomicMin into codes[] (pre-filled
// with VALIDATE_CLEAN): a minimum does not depend on the order of the waves.
struct AccTile {
    fp (*tile)[64];
    unsigned lane;
    __device__ __forceinline__ void add(int i, fp flag, fp val) { tile[i][lane] = fp_add(tile[i][lane], fp_mul(flag, val)); }
};
// the 19 public-input values of SchnorrAir at row q of signature block t (trace_gen.hip, k_schnorr_aux_columns) from the statement's
// messages [n_sig][28]: the public key on every row, the message chunk absorbed after rows 7, 15, 23, 31
__device__ __forceinline__ fp schnorr_aux_value(const fp *__restrict__ messages, size_t t, unsigned q, int j) {
    const fp *m = messages + 28 * t;
    if (j < 12) return m[j];
    return (q < 32 && (q & 7) == 7) ? m[(j - 12) + 7 * (q >> 3)] : 0;
}
// one part of SchnorrAir as a real call: the kernel's register budget is the largest part's, not the sum of the four
template <int PART>
__device__ __noinline__ void validate_schnorr_part(fp (*tile)[64], unsigned lane, const Frame f, const Frame fr, const fp *ax) {
    AccTile acc{tile, lane};
    schnorr_transitions<PART>(acc, f, fr, ax, 64);
}
template <int AIR, int NC>
__global__ __launch_bounds__(64) void k_validate_frames(ValidateParams p) {
    __shared__ fp tile[NC][64];
    __shared__ fp aux[AIR == 2 ? 19 : 1][64]; // SchnorrAir: the public-input values of the lane's row
    const unsigned lane = threadIdx.x;
    const size_t n = (size_t)1 << p.log_n, r = blockIdx.x * (size_t)64 + lane;
    if (r + 1 >= n) return; // the last row is only ever the `next` of frame n - 2
#pragma unroll 1
    for (int i = 0; i < NC; i++) tile[i][lane] = 0;
    const unsigned cycle_len = 1u << p.log_cycle, q = (unsigned)(r & (cycle_len - 1));
    Frame f;
    f.n = n;
    f.cur_p = p.trace + r;
    f.next_p = p.trace + r + 1;
    f.per_p = p.per + q;
    f.pcycle = cycle_len;
    AccTile acc{tile, lane};
    if constexpr (AIR == 0) evaluate_transition(acc, f);
    else if constexpr (AIR == 1) merkle_transitions(acc, f);
    else if constexpr (AIR == 3) range_transitions(acc, f);
    else if constexpr (AIR == 4) rescue_transitions(acc, f);
    else {
#pragma unroll 1
        for (int j = 0; j < 19; j++) aux[j][lane] = schnorr_aux_value(p.messages, r >> p.log_cycle, q, j);
        Frame fr = f;
        fr.per_p = f.per_p - (size_t)(P_ARK - 8) * cycle_len;
        validate_schnorr_part<0>(tile, lane, f, fr, &aux[0][lane]);
        validate_schnorr_part<1>(tile, lane, f, fr, &aux[0][lane]);
        validate_schnorr_part<2>(tile, lane, f, fr, &aux[0][lane]);
        validate_schnorr_part<3>(tile, lane, f, fr, &aux[0][lane]);
    }
#pragma unroll 1
    for (int i = 0; i < NC; i++)
        if (tile[i][lane] != 0) {
            atomicMin(p.codes + (r >> p.log_cycle), q * (unsigned)NC + (unsigned)i);
            break;
        }
}
// summary[0] = the first cycle with a violated frame (pre-filled with VALIDATE_CLEAN), summary[2] = the number of such cycles (pre-filled 0)
__global__ void k_validate_summary(const uint32_t *__restrict__ codes, uint32_t *__restrict__ summary, unsigned n_cycles) {
    const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cycles || codes[c] == VALIDATE_CLEAN) return;
    atomicMin(summary, c);
    atomicAdd(summary + 2, 1u);
}
// Boundary entries: thread (x, y) checks occurrence x of entry y: register `reg` at step first + x * stride against `value`, or against
// seq[entry.seq * n_occ + x] for a sequence entry.  summary[1] = min over the failures of entry << 24 | step (steps are below 2^24):
// the lowest failing entry and its lowest failing step.
__global__ void k_validate_boundary(const fp *__restrict__ trace, const ValidateEntry *__restrict__ entries, const fp *__restrict__ seq,
                                    uint32_t *__restrict__ summary, unsigned log_n) {
    const ValidateEntry e = entries[blockIdx.y];
    const size_t n = (size_t)1 << log_n;
    const unsigned n_occ = e.stride ? (unsigned)(n / e.stride) : 1u;
    const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_occ) return;
    const size_t step = e.first + (size_t)x * e.stride;
    if (step >= n) return;
    const fp want = e.seq >= 0 ? seq[(size_t)e.seq * n_occ + x] : e.value;
    if (trace[(size_t)e.reg * n + step] != want) atomicMin(summary + 1, (blockIdx.y << 24) | (unsigned)step);
}
// frame r of the trace as one free-standing frame of launch_eval_frames_air: dst = cur[width] | next[width] | per[n_per (+ 19 for SchnorrAir)]
__global__ void k_validate_gather_frame(ValidateParams p, fp *__restrict__ dst, size_t r, unsigned width, unsigned n_per) {
    const size_t n = (size_t)1 << p.log_n;
    const unsigned cycle_len = 1u << p.log_cycle, q = (unsigned)(r & (cycle_len - 1));
    const unsigned i = threadIdx.x;
    if (i < width) {
        dst[i] = p.trace[(size_t)i * n + r];
        dst[width + i] = p.trace[(size_t)i * n + r + 1];
    }
    if (i < n_per) dst[2 * width + i] = p.per[(size_t)i * cycle_len + q];
    if (p.messages && i < 19) dst[2 * width + n_per + i] = schnorr_aux_value(p.messages, r >> p.log_cycle, q, (int)i);
}
hipError_t launch_validate_frames(int air, const ValidateParams &p, hipStream_t stream) {
    const size_t n = (size_t)1 << p.log_n;
    if (p.log_cycle > p.log_n || n < 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (air == 0) hipLaunchKernelGGL((k_validate_frames<0, 115>), grid, block, 0, stream, p);
    else if (air == 1) hipLaunchKernelGGL((k_validate_frames<1, 106>), grid, block, 0, stream, p);
    else if (air == 2) hipLaunchKernelGGL((k_validate_frames<2, 56>), grid, block, 0, stream, p);
    else if (air == 3) hipLaunchKernelGGL((k_validate_frames<3, 2>), grid, block, 0, stream, p);
    else if (air == 4) hipLaunchKernelGGL((k_validate_frames<4, 14>), grid, block, 0, stream, p);
    else return hipErrorInvalidValue;
    const unsigned n_cycles = 1u << (p.log_n - p.log_cycle);
    hipLaunchKernelGGL(k_validate_summary, dim3((n_cycles + 255) / 256), dim3(256), 0, stream, p.codes, p.summary, n_cycles);
    return hipGetLastError();
}
hipError_t launch_validate_boundary(const ValidateParams &p, const ValidateEntry *d_entries, unsigned n_entries, const uint64_t *d_seq, unsigned max_occ,
                                    hipStream_t stream) {
    if (n_entries == 0 || n_entries > 255 || max_occ == 0 || p.log_n > 24) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_validate_boundary, dim3((max_occ + 255) / 256, n_entries), dim3(256), 0, stream, p.trace, d_entries, d_seq, p.summary, p.log_n);
    return hipGetLastError();
}
hipError_t launch_validate_gather_frame(const ValidateParams &p, uint64_t *d_dst, size_t r, unsigned width, unsigned n_per, hipStream_t stream) {
    if (r + 1 >= ((size_t)1 << p.log_n) || width > 128 || n_per > 128) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_validate_gather_frame, dim3(1), dim3(128), 0, stream, p, d_dst, r, width, n_per);
    return hipGetLastError();
}

} // namespace cs
