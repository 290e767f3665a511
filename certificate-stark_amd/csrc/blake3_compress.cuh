// The scalar BLAKE3 compression (one lane, one block), shared by the commitment kernels (blake3.hip) and the verifier (verify.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "blake3_quad.cuh"

namespace cs {
namespace {

// message word indices for each of the 7 rounds (the BLAKE3 permutation applied repeatedly)
#define B3_ROUND(m, i0, i1, i2, i3, i4, i5, i6, i7, i8, i9, i10, i11, i12, i13, i14, i15) \
    B3_G(s0, s4, s8, s12, m[i0], m[i1]) B3_G(s1, s5, s9, s13, m[i2], m[i3])               \
    B3_G(s2, s6, s10, s14, m[i4], m[i5]) B3_G(s3, s7, s11, s15, m[i6], m[i7])             \
    B3_G(s0, s5, s10, s15, m[i8], m[i9]) B3_G(s1, s6, s11, s12, m[i10], m[i11])           \
    B3_G(s2, s7, s8, s13, m[i12], m[i13]) B3_G(s3, s4, s9, s14, m[i14], m[i15])

// cv <- first 8 words of compress(cv, m, counter = 0, block_len, flags)
__device__ __forceinline__ void compress(uint32_t (&cv)[8], const uint32_t (&m)[16], uint32_t block_len, uint32_t flags) {
    uint32_t s0 = cv[0], s1 = cv[1], s2 = cv[2], s3 = cv[3], s4 = cv[4], s5 = cv[5], s6 = cv[6], s7 = cv[7];
    uint32_t s8 = IV0, s9 = IV1, s10 = IV2, s11 = IV3, s12 = 0, s13 = 0, s14 = block_len, s15 = flags;
    B3_ROUND(m, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    B3_ROUND(m, 2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
    B3_ROUND(m, 3, 4, 10, 12, 13, 2, 7, 14, 6, 5, 9, 0, 11, 15, 8, 1)
    B3_ROUND(m, 10, 7, 12, 9, 14, 3, 13, 15, 4, 0, 11, 2, 5, 8, 1, 6)
    B3_ROUND(m, 12, 13, 9, 11, 15, 10, 14, 8, 7, 2, 5, 3, 0, 1, 6, 4)
    B3_ROUND(m, 9, 14, 11, 5, 8, 12, 15, 1, 13, 3, 0, 10, 2, 6, 4, 7)
    B3_ROUND(m, 11, 15, 5, 0, 1, 9, 8, 6, 14, 10, 2, 12, 3, 4, 7, 13)
    cv[0] = s0 ^ s8; cv[1] = s1 ^ s9; cv[2] = s2 ^ s10; cv[3] = s3 ^ s11;
    cv[4] = s4 ^ s12; cv[5] = s5 ^ s13; cv[6] = s6 ^ s14; cv[7] = s7 ^ s15;
}

} // namespace
} // namespace cs
