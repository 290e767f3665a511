// The kernels that carry polynomials between cosets as coefficient vectors, reachable from a test one at a time
// (include/cstark_debug_coset.h): the extension from the even to the odd cosets, plain, windowed and merged, the coset combination, the
// high part of the final addition with its merged form, and the data mover of the sharded path.  Every entry point checks its arguments
// on the host first -- shapes, windows, table indices, the kernels' reach against the stated buffer sizes -- and refuses before anything
// is launched; then it is the product's own host function over power tables built by cs::ntt_power_table, called on the context's
// stream and followed by a synchronisation.
#include <hip/hip_runtime.h>
#include "../../../include/cstark_debug_coset.h"
#include "../constraints.h"
#include "../ctx.h"
#include "../hostfield.h"
#include "../ntt.h"

namespace {
constexpr int REFUSED = (int)hipErrorInvalidValue;
constexpr uint32_t MAX_TABLES = 64;
static_assert(CSTARK_DEBUG_MERGE_FAMILIES == cs::COSET_MERGE_MAX_FAMILIES && CSTARK_DEBUG_MERGE_TERMS == cs::COSET_MERGE_MAX_TERMS, "the header's limits");
bool aligned(const void *p) { return ((uintptr_t)p & 7) == 0; }
bool canonical(uint64_t word) { return word < cs::host::P; }
// [a, a + na) and [b, b + nb) words share nothing
bool apart(const uint64_t *a, size_t na, const uint64_t *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa + na * 8 <= pb || pb + nb * 8 <= pa;
}
// the power tables of one call, freed with it
struct Tables {
    uint64_t *t[2] = {nullptr, nullptr};
    ~Tables() { for (uint64_t *p : t) if (p) (void)hipFree(p); }
    hipError_t build(int i, size_t entries, uint64_t base, hipStream_t st) {
        hipError_t e = hipMalloc((void **)&t[i], entries * 8);
        return e != hipSuccess ? e : cs::ntt_power_table(t[i], entries, base, st);
    }
    // winv_4n in t[0], w_8n in t[1]: what both extension kernels read
    hipError_t build_extension(unsigned log_n, hipStream_t st) {
        hipError_t e = build(0, (size_t)4 << log_n, cs::host::inv(cs::host::root_of_unity(log_n + 2)), st);
        return e != hipSuccess ? e : build(1, (size_t)8 << log_n, cs::host::root_of_unity(log_n + 3), st);
    }
};
int finish(hipError_t e, hipStream_t st) {
    const hipError_t s = hipStreamSynchronize(st); // the tables are freed after the kernels that read them
    return e != hipSuccess ? (int)e : (int)s;
}
void copy_term(cstark_debug_merge_term *out, const cs::CosetMergeTerm &t) {
    for (int i = 0; i < 4; i++) { out->c[i][0] = t.c[i][0]; out->c[i][1] = t.c[i][1]; }
    out->table = t.table;
    out->r = t.r;
}
uint64_t quarter() { return cs::host::inv(cs::host::from_u64(4)); }
uint64_t half() { return cs::host::inv(cs::host::from_u64(2)); }
} // namespace

extern "C" int cstark_debug_even_to_odd(void *ctx, const uint64_t *d_in, size_t in_words, uint64_t *d_out, size_t out_words, uint32_t log_n, uint32_t tables,
                                        uint32_t kc0, uint32_t nkc) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_in || !d_out || !aligned(d_in) || !aligned(d_out)) return REFUSED;
    if (nkc == 0 || kc0 > 4 || nkc > 4 - kc0 || tables == 0 || tables > MAX_TABLES || log_n < 6 || log_n + 3 > cs::NTT_MAX_LOG_N) return REFUSED;
    const size_t need = ((size_t)4 * tables) << log_n;
    if (in_words < need || out_words < need || !apart(d_in, need, d_out, need)) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    Tables tb;
    hipError_t e = tb.build_extension(log_n, c->stream);
    if (e == hipSuccess) e = cs::coset_even_to_odd(d_in, d_out, log_n, tables, tb.t[0], tb.t[1], quarter(), c->stream, kc0, nkc);
    return finish(e, c->stream);
}

extern "C" int cstark_debug_even_to_odd_merged(void *ctx, const uint64_t *d_in, size_t in_words, uint64_t *d_out, size_t out_words, uint64_t *d_raw,
                                               size_t raw_words, uint32_t log_n, uint32_t sets, const cstark_debug_merge_desc *desc,
                                               cstark_debug_merge_term *terms_out) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_in || !d_out || !desc || !aligned(d_in) || !aligned(d_out) || !aligned(d_raw)) return REFUSED;
    if (log_n < 6 || log_n + 3 > cs::NTT_MAX_LOG_N || sets == 0 || sets > 8) return REFUSED;
    if (desc->families == 0 || desc->families > CSTARK_DEBUG_MERGE_FAMILIES || desc->tables_per_set == 0 || desc->tables_per_set > MAX_TABLES) return REFUSED;
    if (desc->raw_family < -1 || desc->raw_family >= (int32_t)desc->families || !canonical(desc->base) || (desc->k0 != 1 && desc->k0 != 2)) return REFUSED;
    for (uint32_t f = 0; f < desc->families; f++) {
        if (desc->terms[f] == 0 || desc->terms[f] > CSTARK_DEBUG_MERGE_TERMS) return REFUSED;
        for (uint32_t t = 0; t < desc->terms[f]; t++)
            if (desc->table[f][t] >= desc->tables_per_set) return REFUSED;
    }
    const size_t n = (size_t)1 << log_n, need_in = (size_t)4 * sets * desc->tables_per_set * n, need_out = (size_t)4 * sets * desc->families * n;
    const bool raw = d_raw && desc->raw_family >= 0;
    const size_t need_raw = raw ? (size_t)sets * desc->terms[desc->raw_family] * n : 0;
    if (in_words < need_in || out_words < need_out || raw_words < need_raw || !apart(d_in, need_in, d_out, need_out)) return REFUSED;
    if (raw && (!apart(d_in, need_in, d_raw, need_raw) || !apart(d_out, need_out, d_raw, need_raw))) return REFUSED;
    cs::CosetMergeDesc d{};
    d.families = desc->families;
    d.tables_per_set = desc->tables_per_set;
    d.raw_family = desc->raw_family;
    for (uint32_t f = 0; f < desc->families; f++) {
        d.terms[f] = desc->terms[f];
        for (uint32_t t = 0; t < desc->terms[f]; t++) {
            d.term[f][t] = cs::coset_merge_term(desc->table[f][t], desc->exponent[f][t], log_n, desc->base, desc->k0);
            if (d.term[f][t].r >= n) return REFUSED;
        }
    }
    if (terms_out)
        for (uint32_t f = 0; f < desc->families; f++)
            for (uint32_t t = 0; t < desc->terms[f]; t++) copy_term(&terms_out[f * CSTARK_DEBUG_MERGE_TERMS + t], d.term[f][t]);
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    Tables tb;
    hipError_t e = tb.build_extension(log_n, c->stream);
    if (e == hipSuccess) e = cs::coset_even_to_odd_merged(d_in, d_out, log_n, sets, d, tb.t[0], tb.t[1], quarter(), d_raw, c->stream);
    return finish(e, c->stream);
}

extern "C" int cstark_debug_coset_combine(void *ctx, const uint64_t *d_b, uint64_t *d_h, size_t words, uint32_t log_n, uint32_t log_b, uint32_t tables) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_b || !d_h || !aligned(d_b) || !aligned(d_h)) return REFUSED;
    if (log_b < 1 || log_b > 3 || log_n < 6 || log_n + log_b > cs::NTT_MAX_LOG_N || tables == 0 || tables > MAX_TABLES) return REFUSED;
    const size_t need = (size_t)tables << (log_n + log_b);
    if (words < need || !apart(d_b, need, d_h, need)) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    Tables tb;
    hipError_t e = tb.build(0, (size_t)1 << (log_n + log_b), cs::host::inv(cs::host::root_of_unity(log_n + log_b)), c->stream);
    if (e == hipSuccess)
        e = cs::coset_combine(d_b, d_h, log_n, log_b, tb.t[0], cs::host::inv(cs::host::from_u64(1ull << log_b)), c->stream, tables);
    return finish(e, c->stream);
}

extern "C" int cstark_debug_final_hi(void *ctx, const uint64_t *d_odd, size_t odd_words, const uint64_t *d_direct, size_t direct_words, uint64_t *d_hi,
                                     size_t hi_words, uint32_t log_n, uint32_t rows, uint32_t first, uint32_t per_set, uint32_t tables_per_set) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_odd || !d_direct || !d_hi || !aligned(d_odd) || !aligned(d_direct) || !aligned(d_hi)) return REFUSED;
    if (log_n < 8 || log_n > 20 || rows == 0 || rows > 64 || per_set == 0 || rows % per_set || tables_per_set > MAX_TABLES || first > tables_per_set ||
        per_set > tables_per_set - first)
        return REFUSED;
    const size_t need_odd = ((size_t)(rows / per_set) * tables_per_set) << log_n, need = (size_t)rows << log_n;
    if (odd_words < need_odd || direct_words < need || hi_words < need) return REFUSED;
    if (!apart(d_odd, need_odd, d_hi, need) || !apart(d_direct, need, d_hi, need)) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    return finish(cs::launch_final_hi(d_odd, d_direct, d_hi, half(), log_n, rows, first, per_set, tables_per_set, c->stream), c->stream);
}

extern "C" int cstark_debug_final_hi_merge(void *ctx, const uint64_t *d_tco, const uint64_t *d_qco, size_t in_words, uint64_t *d_out, size_t out_words,
                                           uint32_t log_n, uint32_t m, uint64_t e, uint64_t base, uint32_t k0, cstark_debug_merge_term *term_out) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_tco || !d_qco || !d_out || !aligned(d_tco) || !aligned(d_qco) || !aligned(d_out)) return REFUSED;
    if (log_n < 8 || log_n + 3 > cs::NTT_MAX_LOG_N || m == 0 || m > (uint32_t)cs::CE_MAX_SETS || !canonical(base) || (k0 != 1 && k0 != 2)) return REFUSED;
    const size_t need_in = ((size_t)2 * m) << log_n, need_out = ((size_t)3 * m) << log_n;
    if (in_words < need_in || out_words < need_out || !apart(d_tco, need_in, d_out, need_out) || !apart(d_qco, need_in, d_out, need_out)) return REFUSED;
    const cs::CosetMergeTerm tm = cs::coset_merge_term(0, e, log_n, base, k0);
    if (tm.r >= ((size_t)1 << log_n)) return REFUSED;
    if (term_out) copy_term(term_out, tm);
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    cs::CeParams p{}; // the launcher reads log_n and m alone
    p.log_n = log_n;
    p.m = m;
    return finish(cs::launch_final_hi_merge(p, d_tco, d_qco, d_out, tm, half(), c->stream), c->stream);
}

extern "C" int cstark_debug_shard_combine(void *ctx, const uint64_t *d_parts, size_t parts_words, uint64_t *d_out, size_t out_words, uint32_t log_n,
                                          uint32_t nkc) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_parts || !d_out || !aligned(d_parts) || !aligned(d_out) || (nkc != 1 && nkc != 2) || log_n < 8 || log_n > 20) return REFUSED;
    const size_t need_parts = ((size_t)(4 / nkc) * (nkc + 4)) << log_n, need_out = (size_t)8 << log_n;
    if (parts_words < need_parts || out_words < need_out || !apart(d_parts, need_parts, d_out, need_out)) return REFUSED;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    return finish(cs::launch_shard_combine(d_parts, d_out, log_n, nkc, c->stream), c->stream);
}
