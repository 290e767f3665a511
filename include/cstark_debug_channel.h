/* cstark_debug_channel.h -- TEST-ONLY, served by libcstark_debug.so like cstark_debug_ood.h: thin wrappers over internal host
 * functions of the product library, so that a test chooses the inputs of the kernels that branch on hash output -- the device
 * Fiat-Shamir channel (csrc/channel.hip), the FRI layer coins and the proof-of-work searches (csrc/blake3.hip, csrc/sha3.hip,
 * csrc/prove.hip).  `ctx` is a cstark_ctx; every call runs on the context's stream and synchronises it.
 * Return: the hipError_t of the wrapped function (0 = hipSuccess, 1 = hipErrorInvalidValue: refused, nothing launched), except
 * cstark_debug_grind_search, which returns a cstark_status.
 */
#ifndef CSTARK_DEBUG_CHANNEL_H
#define CSTARK_DEBUG_CHANNEL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* cs::ChanStep (csrc/channel.h) field by field, as a C struct: see there for what every field means.  Pointers are device memory but
 * `prefix`, which is part of the struct. */
typedef struct cstark_debug_chan_absorb {
    uint32_t kind, count;
    const void *ptr;
    uint64_t value;
    uint8_t *copy_out;
} cstark_debug_chan_absorb;
typedef struct cstark_debug_chan_step {
    uint32_t *seed;
    uint32_t init, prefix_len, npub;
    uint8_t prefix[32];
    const uint64_t *pub;
    cstark_debug_chan_absorb absorb[3];
    uint32_t draw, count, a, b, stride, per;
    uint32_t m, set_stride;
    uint64_t *out, *out2;
    uint64_t w;
    uint32_t log_domain, log_f, n_layers, slot;
    uint32_t *pos, *cnt;
} cstark_debug_chan_step;
/* cs::channel_step: one launch of k_chan_step */
int cstark_debug_channel_step(void *ctx, const cstark_debug_chan_step *step);
/* m = 1: cs::fri_coin, m = 2, 3: cs::fri_coin_ext (any other m is passed to it and refused).  d_seed [8 words] in and out, d_root
 * [32 bytes], d_alpha [m words] out, d_root_out [8 words] out. */
int cstark_debug_fri_coin(void *ctx, uint32_t m, uint32_t *d_seed, const uint8_t *d_root, uint64_t *d_alpha, uint32_t *d_root_out);
/* One chunk of a proof-of-work search: nonces [base, base + count).
 *   form 0  cs::grind_chunk: `seeds` = 32 bytes of HOST memory, batch ignored; d_found[0] is preset to ~0 by the function itself
 *   form 1  cs::grind_batch_chunk: `seeds` = [batch][8] 32-bit words of device memory
 *   form 2  cs::grind_batch_chunk_sha3: `seeds` = [batch][4] 64-bit words of device memory
 * Forms 1 and 2 read and lower d_found[batch] as the caller preset it. */
int cstark_debug_grind_chunk(void *ctx, uint32_t form, const void *seeds, uint32_t batch, uint64_t base, uint64_t count, uint32_t bits,
                             unsigned long long *d_found);
/* The chunk loop of the prover's grind_nonce (csrc/ctx.h, grind_search) with a chunk of the caller's choice; seed: 32 bytes of host
 * memory; hash_fn 0 = Blake3, 1 = Sha3; d_found: 5 device words of scratch.  Return: cstark_status. */
int cstark_debug_grind_search(void *ctx, unsigned long long *d_found, const uint8_t *seed, uint32_t hash_fn, uint32_t bits, uint64_t chunk,
                              uint64_t *nonce_out);
#ifdef __cplusplus
}
#endif
#endif
