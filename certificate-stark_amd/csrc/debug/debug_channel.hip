// The kernels that branch on hash output, reachable from a test with inputs of its choice (include/cstark_debug_channel.h): the device
// Fiat-Shamir channel, the FRI layer coins, the proof-of-work chunk searches and the chunk loop of the prover's grind_nonce.  Every
// entry point is the product's own host function, called on the context's stream and followed by a synchronisation.
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../../include/cstark_debug_channel.h"
#include "../blake3.h"
#include "../channel.h"
#include "../ctx.h"

namespace {
int finish(hipError_t e, hipStream_t st) {
    if (e != hipSuccess) return (int)e;
    return (int)hipStreamSynchronize(st);
}
} // namespace

extern "C" int cstark_debug_channel_step(void *ctx, const cstark_debug_chan_step *d) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d) return (int)hipErrorInvalidValue;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    cs::ChanStep s{};
    s.seed = d->seed;
    s.init = d->init; s.prefix_len = d->prefix_len; s.npub = d->npub;
    memcpy(s.prefix, d->prefix, sizeof s.prefix);
    s.pub = d->pub;
    for (int k = 0; k < 3; k++) {
        s.absorb[k].kind = d->absorb[k].kind; s.absorb[k].count = d->absorb[k].count; s.absorb[k].ptr = d->absorb[k].ptr;
        s.absorb[k].value = d->absorb[k].value; s.absorb[k].copy_out = d->absorb[k].copy_out;
    }
    s.draw = d->draw; s.count = d->count; s.a = d->a; s.b = d->b; s.stride = d->stride; s.per = d->per;
    s.m = d->m; s.set_stride = d->set_stride;
    s.out = d->out; s.out2 = d->out2;
    s.w = d->w;
    s.log_domain = d->log_domain; s.log_f = d->log_f; s.n_layers = d->n_layers; s.slot = d->slot;
    s.pos = d->pos; s.cnt = d->cnt;
    return finish(cs::channel_step(s, c->stream), c->stream);
}

extern "C" int cstark_debug_fri_coin(void *ctx, uint32_t m, uint32_t *d_seed, const uint8_t *d_root, uint64_t *d_alpha, uint32_t *d_root_out) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_seed || !d_root || !d_alpha || !d_root_out) return (int)hipErrorInvalidValue;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    if (m == 1) return finish(cs::fri_coin(d_seed, d_root, d_alpha, d_root_out, c->stream), c->stream);
    return finish(cs::fri_coin_ext(d_seed, d_root, d_alpha, d_root_out, m, c->stream), c->stream);
}

extern "C" int cstark_debug_grind_chunk(void *ctx, uint32_t form, const void *seeds, uint32_t batch, uint64_t base, uint64_t count, uint32_t bits,
                                        unsigned long long *d_found) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !seeds || !d_found || form > 2 || count == 0 || count > ((uint64_t)1 << 28) || (form != 0 && (batch == 0 || batch > 1024)))
        return (int)hipErrorInvalidValue;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    if (form == 0) return finish(cs::grind_chunk((const uint8_t *)seeds, base, count, bits, d_found, c->stream), c->stream);
    if (form == 1) return finish(cs::grind_batch_chunk((const uint32_t *)seeds, batch, base, count, bits, d_found, c->stream), c->stream);
    return finish(cs::grind_batch_chunk_sha3((const uint64_t *)seeds, batch, base, count, bits, d_found, c->stream), c->stream);
}

extern "C" int cstark_debug_grind_search(void *ctx, unsigned long long *d_found, const uint8_t *seed, uint32_t hash_fn, uint32_t bits, uint64_t chunk,
                                         uint64_t *nonce_out) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_found || !seed || !nonce_out || hash_fn > 1 || chunk == 0 || chunk > ((uint64_t)1 << 28)) return CSTARK_ERR_INVALID_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CSTARK_ERR_HIP;
    return cs::grind_search(c->stream, d_found, seed, hash_fn, bits, chunk, nonce_out);
}
