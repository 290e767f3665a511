// The commitment and opening kernels, reachable from a test with layouts and positions of its choice (include/cstark_debug_commit.h):
// row hashes in block order, the batched tables and trees, the opening gathers of a proof and of the batched range prover.  Every entry
// point checks its arguments on the host first -- shapes, every position, the kernels' reach against the stated buffer sizes -- and
// refuses before anything is launched; then it is the product's own host function, called on the context's stream and followed by a
// synchronisation.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../../include/cstark_debug_commit.h"
#include "../blake3.h"
#include "../ctx.h"
#include "../range_batch.h"

namespace {
constexpr int REFUSED = (int)hipErrorInvalidValue;
int finish(hipError_t e, hipStream_t st) {
    if (e != hipSuccess) return (int)e;
    return (int)hipStreamSynchronize(st);
}
bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// the checks shared by the two batched-tree entries: the trees [batch] at d_nodes + t stride, 2 L digests each
bool trees_fit(const uint8_t *d_nodes, size_t nodes_bytes, uint32_t log_leaves, uint32_t batch, size_t stride) {
    if (!d_nodes || !aligned(d_nodes, 16) || log_leaves < 1 || log_leaves > 11 || batch == 0 || batch > 1024) return false;
    const size_t tree = (size_t)64 << log_leaves;
    return stride >= tree && stride % 32 == 0 && nodes_bytes >= (size_t)(batch - 1) * stride + tree;
}
} // namespace

extern "C" int cstark_debug_hash_rows_slots(void *ctx, uint32_t hash_fn, const uint64_t *d_table, size_t table_words, uint8_t *d_leaves, size_t leaves_bytes,
                                            uint32_t width, uint32_t log_n, uint32_t log_b, uint32_t log_s, uint32_t k0, uint32_t nk) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_table || !d_leaves || !aligned(d_table, 8) || !aligned(d_leaves, 16) || hash_fn > 1) return REFUSED;
    if (width == 0 || width > 128 || log_n > 20 || log_b > 4 || log_s > log_b || nk == 0 || k0 > (1u << log_b) || nk > (1u << log_b) - k0) return REFUSED;
    if (table_words < ((size_t)nk * width << log_n) || leaves_bytes < ((size_t)32 << (log_n + log_b))) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    if (hash_fn == 1) return finish(cs::hash_rows_sha3(d_table, d_leaves, width, log_n, log_b, k0, nk, c->stream, log_s), c->stream);
    return finish(cs::hash_rows(d_table, d_leaves, width, log_n, log_b, k0, nk, c->stream, log_s), c->stream);
}

extern "C" int cstark_debug_commit_batch(void *ctx, uint32_t hash_fn, const uint64_t *d_table, size_t table_words, uint8_t *d_nodes, size_t nodes_bytes,
                                         uint32_t gw, uint32_t log_n, uint32_t log_b, uint32_t batch, size_t stride) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_table || !aligned(d_table, 8) || hash_fn > 1 || gw == 0 || gw > 8 || log_n > 11 || log_b > 4) return REFUSED;
    const uint32_t log_leaves = log_n + log_b;
    if (!trees_fit(d_nodes, nodes_bytes, log_leaves, batch, stride)) return REFUSED;
    if (table_words < ((size_t)gw * batch << log_leaves)) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    uint8_t *leaves = d_nodes + ((size_t)32 << log_leaves);
    hipError_t e = hash_fn == 1 ? cs::hash_rows_batch_sha3(d_table, leaves, gw, gw * batch, log_n, log_b, batch, stride, c->stream)
                                : cs::hash_rows_batch(d_table, leaves, gw, gw * batch, log_n, log_b, batch, stride, c->stream);
    if (e == hipSuccess)
        e = hash_fn == 1 ? cs::merkle_build_batch_sha3(d_nodes, log_leaves, batch, stride, c->stream) : cs::merkle_build_batch(d_nodes, log_leaves, batch, stride, c->stream);
    return finish(e, c->stream);
}

extern "C" int cstark_debug_merkle_batch(void *ctx, uint32_t hash_fn, uint8_t *d_nodes, size_t nodes_bytes, uint32_t log_leaves, uint32_t batch, size_t stride) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || hash_fn > 1 || !trees_fit(d_nodes, nodes_bytes, log_leaves, batch, stride)) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    if (hash_fn == 1) return finish(cs::merkle_build_batch_sha3(d_nodes, log_leaves, batch, stride, c->stream), c->stream);
    return finish(cs::merkle_build_batch(d_nodes, log_leaves, batch, stride, c->stream), c->stream);
}

extern "C" int cstark_debug_gather(void *ctx, const cstark_debug_gather_job *jobs, uint32_t n_jobs) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !jobs || n_jobs == 0 || n_jobs > 32) return REFUSED;
    // host block of what the kernel reads on the device: per job its positions, then one word per job for the device-side count
    std::vector<uint32_t> h;
    size_t pos_at[32];
    for (uint32_t i = 0; i < n_jobs; i++) {
        const cstark_debug_gather_job &j = jobs[i];
        if (!j.d_src || !j.d_out || j.count > 4096 || (j.count && !j.positions) || j.dcount > (int64_t)j.count) return REFUSED;
        uint64_t domain;
        if (j.paths) {
            if (j.log_leaves < 1 || j.log_leaves > 28 || j.lvl0 > j.log_leaves || !aligned(j.d_src, 16) || !aligned(j.d_out, 16)) return REFUSED;
            domain = (uint64_t)1 << j.log_leaves;
            if (j.src_bytes < 64 * domain || j.out_bytes < (size_t)j.count * j.log_leaves * 32) return REFUSED;
        } else {
            if (j.width == 0 || j.width > 1024 || j.log_n > 24 || j.log_b > 4 || j.log_s > j.log_b || !aligned(j.d_src, 8) || !aligned(j.d_out, 8)) return REFUSED;
            domain = (uint64_t)1 << (j.log_n + j.log_b);
            if (j.src_bytes < 8 * domain * j.width || j.out_bytes < (size_t)j.count * j.width * 8) return REFUSED;
        }
        for (uint32_t q = 0; q < j.count; q++)
            if (j.positions[q] >= domain) return REFUSED;
        pos_at[i] = h.size();
        h.insert(h.end(), j.positions, j.positions + j.count);
    }
    const size_t counts_at = h.size();
    for (uint32_t i = 0; i < n_jobs; i++) h.push_back(jobs[i].dcount >= 0 ? (uint32_t)jobs[i].dcount : jobs[i].count);
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    uint32_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, h.size() * 4);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    int rc = (int)e;
    if (e == hipSuccess) {
        cstark_gather_desc g[32];
        for (uint32_t i = 0; i < n_jobs; i++) {
            const cstark_debug_gather_job &j = jobs[i];
            g[i] = cstark_gather_desc{j.d_src, j.d_out, d + pos_at[i], j.dcount >= 0 ? d + counts_at + i : nullptr, j.paths ? 1u : 0u,
                                      j.paths ? j.log_leaves : j.width, j.log_n, j.log_b, j.log_s, j.count, j.lvl0};
        }
        rc = gather_jobs_launch(c, g, n_jobs);
        const int rs = (int)hipStreamSynchronize(c->stream);
        if (rc == 0) rc = rs;
    }
    (void)hipFree(d);
    return rc;
}

extern "C" int cstark_debug_range_open(void *ctx, const cstark_debug_rb_open *o) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !o || o->batch == 0 || o->batch > 1024 || o->nq == 0 || o->nq > 128 || o->n_layers > 1) return REFUSED;
    const size_t B = o->batch, nq = o->nq;
    if (!o->d_lde || !o->d_clde || !o->d_tnodes || !o->d_cnodes || !o->pos || !o->d_out) return REFUSED;
    if (o->lde_words < 8 * 2 * B * 64 || o->clde_words < 8 * 2 * B * 64 || o->tnodes_bytes < B * 1024 * 32 || o->cnodes_bytes < B * 1024 * 32) return REFUSED;
    if (!aligned(o->d_lde, 8) || !aligned(o->d_clde, 8) || !aligned(o->d_tnodes, 16) || !aligned(o->d_cnodes, 16) || !aligned(o->d_out, 16)) return REFUSED;
    if (o->n_layers) {
        if (!o->d_layer || !o->d_lnodes || !o->lpos || !o->lcount || !aligned(o->d_layer, 8) || !aligned(o->d_lnodes, 16)) return REFUSED;
        if (o->layer_words < B * 512 || o->lnodes_bytes < B * 256 * 32) return REFUSED;
    }
    // the sections of a slot: {offset, bytes, alignment}
    const size_t sec[6][3] = {{o->trows, nq * 16, 8},   {o->tpaths, nq * 9 * 32, 16}, {o->crows, nq * 16, 8},
                              {o->cpaths, nq * 9 * 32, 16}, {o->lrows, nq * 32, 8},   {o->lpaths, nq * 7 * 32, 16}};
    if (o->slot % 16 || o->out_bytes / B < o->slot) return REFUSED;
    for (int s = 0; s < (o->n_layers ? 6 : 4); s++)
        if (sec[s][0] % sec[s][2] || sec[s][0] > o->slot || sec[s][1] > o->slot - sec[s][0]) return REFUSED;
    for (size_t i = 0; i < B * nq; i++)
        if (o->pos[i] >= 512 || (o->n_layers && o->lpos[i] >= 128)) return REFUSED;
    for (size_t t = 0; o->n_layers && t < B; t++)
        if (o->lcount[t] > nq) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    // pos | lpos | lcount on the device (zeros where n_layers = 0: never read)
    std::vector<uint32_t> h(2 * B * nq + B, 0);
    for (size_t i = 0; i < B * nq; i++) { h[i] = o->pos[i]; if (o->n_layers) h[B * nq + i] = o->lpos[i]; }
    for (size_t t = 0; o->n_layers && t < B; t++) h[2 * B * nq + t] = o->lcount[t];
    uint32_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, h.size() * 4);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    int rc = (int)e;
    if (e == hipSuccess) {
        const cs::RangeBatchOpen r{o->d_lde, o->d_clde, o->d_layer, o->d_tnodes, o->d_cnodes, o->d_lnodes, d, d + B * nq, d + 2 * B * nq, o->d_out,
                                   o->nq, o->batch, o->n_layers, o->slot, o->trows, o->tpaths, o->crows, o->cpaths, o->lrows, o->lpaths};
        rc = finish(cs::rb_open(r, c->stream), c->stream);
    }
    (void)hipFree(d);
    return rc;
}
