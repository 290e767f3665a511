// Byte-string hashing for the verifier's device transcript (verify.hip): BLAKE3 of any length (chunks with their counters, the
// left-balanced tree merged level by level) and SHA3-256.  Host and device: the host build checks it against hostblake3.h / keccak.cuh.
#pragma once
#include <stdint.h>
#include "keccak.cuh"

namespace cs { namespace vh {

#if defined(__HIPCC__)
#define VH_HD __host__ __device__ __forceinline__
#else
#define VH_HD inline
#endif

enum : uint32_t { B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8 };
VH_HD uint32_t iv(int i) {
    return i == 0 ? 0x6A09E667u : i == 1 ? 0xBB67AE85u : i == 2 ? 0x3C6EF372u : i == 3 ? 0xA54FF53Au : i == 4 ? 0x510E527Fu
         : i == 5 ? 0x9B05688Cu : i == 6 ? 0x1F83D9ABu : 0x5BE0CD19u;
}
VH_HD uint32_t rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }
VH_HD void g(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t mx, uint32_t my) {
    a = a + b + mx; d = rotr(d ^ a, 16); c = c + d; b = rotr(b ^ c, 12);
    a = a + b + my; d = rotr(d ^ a, 8); c = c + d; b = rotr(b ^ c, 7);
}
// cv <- first 8 words of compress(cv, m, counter, block_len, flags)
VH_HD void compress(uint32_t (&cv)[8], uint32_t (&m)[16], uint64_t counter, uint32_t block_len, uint32_t flags) {
    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { s[i] = cv[i]; s[8 + (i & 3)] = iv(i & 3); }
    s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = block_len; s[15] = flags;
#pragma unroll
    for (int r = 0; r < 7; r++) {
        g(s[0], s[4], s[8], s[12], m[0], m[1]); g(s[1], s[5], s[9], s[13], m[2], m[3]);
        g(s[2], s[6], s[10], s[14], m[4], m[5]); g(s[3], s[7], s[11], s[15], m[6], m[7]);
        g(s[0], s[5], s[10], s[15], m[8], m[9]); g(s[1], s[6], s[11], s[12], m[10], m[11]);
        g(s[2], s[7], s[8], s[13], m[12], m[13]); g(s[3], s[4], s[9], s[14], m[14], m[15]);
        if (r < 6) { // the message permutation 2 6 3 10 7 0 4 13 1 11 12 5 9 14 15 8
            const uint32_t t[16] = {m[2], m[6], m[3], m[10], m[7], m[0], m[4], m[13], m[1], m[11], m[12], m[5], m[9], m[14], m[15], m[8]};
#pragma unroll
            for (int i = 0; i < 16; i++) m[i] = t[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = s[i] ^ s[8 + i];
}
// chaining value of chunk `chunk` (len <= 1024 bytes at p); root: the message is this one chunk
VH_HD void b3_chunk(const uint8_t *p, uint32_t len, uint64_t chunk, bool root, uint32_t (&cv)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = iv(i);
    const uint32_t nb = len == 0 ? 1 : (len + 63) / 64;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t bl = len - 64 * b < 64 ? len - 64 * b : 64;
        uint32_t m[16];
#pragma unroll
        for (int w = 0; w < 16; w++) {
            uint32_t v = 0;
            for (int k = 0; k < 4; k++) {
                const uint32_t o = 4 * w + k;
                if (o < bl) v |= (uint32_t)p[64 * b + o] << (8 * k);
            }
            m[w] = v;
        }
        const uint32_t fl = (b == 0 ? B3_CHUNK_START : 0u) | (b + 1 == nb ? (B3_CHUNK_END | (root ? B3_ROOT : 0u)) : 0u);
        compress(cv, m, chunk, bl, fl);
    }
}
VH_HD void b3_parent(const uint32_t *l, const uint32_t *r, bool root, uint32_t (&out)[8]) {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { m[i] = l[i]; m[8 + i] = r[i]; out[i] = iv(i); }
    compress(out, m, 0, 64, B3_PARENT | (root ? B3_ROOT : 0u));
}
// the tree over n > 1 chunk chaining values cvs[0..n) (overwritten), merged level by level -- an odd last node moves up unchanged, which
// gives BLAKE3's left-balanced tree -- with the root flag on the last merge
VH_HD void b3_merge(uint32_t (*cvs)[8], uint32_t n, uint32_t (&out)[8]) {
    while (n > 2) {
        for (uint32_t i = 0; 2 * i + 1 < n; i++) {
            uint32_t t[8];
            b3_parent(cvs[2 * i], cvs[2 * i + 1], false, t);
            for (int k = 0; k < 8; k++) cvs[i][k] = t[k];
        }
        if (n & 1)
            for (int k = 0; k < 8; k++) cvs[n / 2][k] = cvs[n - 1][k];
        n = (n + 1) / 2;
    }
    b3_parent(cvs[0], cvs[1], true, out);
}
// SHA3-256 of len bytes
VH_HD void sha3(const uint8_t *p, uint32_t len, uint64_t (&out)[4]) {
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
    for (uint32_t o = 0;; o += 136) {
        const uint32_t rem = len - o;
        const bool last = rem < 136;
#pragma unroll
        for (int w = 0; w < 17; w++) {
            uint64_t v = 0;
            for (int k = 0; k < 8; k++) {
                const uint32_t i = 8 * w + k;
                uint64_t byte = i < rem ? p[o + i] : 0;
                if (last && i == rem) byte ^= 0x06;
                if (last && i == 135) byte ^= 0x80;
                v |= byte << (8 * k);
            }
            s[w] ^= v;
        }
        keccak::permute(s);
        if (last) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = s[i];
}

}} // namespace cs::vh
