// The lane-per-state-element Rescue permutation shared by the trace kernels (trace_gen.hip) and the ledger's merge kernel
// (ledger.hip): a 14-element state held one element per lane, the MDS products as 128-bit dot products against an LDS exchange row.
#pragma once
#include "rescue.cuh"

namespace cs {

// this lane's row of the MDS matrix against the state in LDS: 128-bit accumulation of the 14 products, one reduction (572 instead of
// 936 issue cycles for 14 reduced products and 13 modular additions)
__device__ __forceinline__ fp mds_row_dot(const fp (&mrow)[14], const fp *xch) {
    Acc128 a = acc_zero();
#pragma unroll
    for (int j = 0; j < 7; j++) acc_mad(a, mrow[j], xch[j]);
    acc_fold(a);
#pragma unroll
    for (int j = 7; j < 14; j++) acc_mad(a, mrow[j], xch[j]);
    acc_fold(a);
    return acc_reduce(a);
}

// One Rescue round on a 14-element state held one element per lane (rescue.rs:246-263).
// `xch` is the state's 14-word LDS exchange row.  Must be called by every lane of the block
// (it synchronises); lanes with active == false only take part in the barriers.
__device__ __forceinline__ fp rescue_round_lane(fp v, fp *xch, const fp (&mrow)[14], int e, int cyc, bool active) {
    fp x = 0;
    if (active) { x = fp_cube(v); xch[e] = x; }
    __syncthreads();
    if (active) x = fp_inv_sbox(fp_add(mds_row_dot(mrow, xch), c_ark[cyc * 28 + e]));
    __syncthreads();
    if (active) xch[e] = x;
    __syncthreads();
    if (active) v = fp_add(mds_row_dot(mrow, xch), c_ark[cyc * 28 + 14 + e]);
    __syncthreads();
    return v;
}

} // namespace cs
