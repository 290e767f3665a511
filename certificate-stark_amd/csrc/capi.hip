// C ABI of the backend (include/cstark.h): context management, cached tables, witness upload and the stage
// entry points.  No torch types, no CPU fallback: without a HIP device every compute entry point returns
// CSTARK_ERR_NO_DEVICE (context creation fails).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <deque>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>
#include "../../include/cstark.h"
#include "air_tx_host.h"
#include "blake3.h"
#include "ctx.h"
#include "constraints.h"
#include "deep.h"
#include "ext.h"
#include "generator_fold.h"
#include "hostfield.h"
#include "ntt.h"
#include "sign_plan.h"
#include "trace_gen.h"

namespace cs { thread_local char g_err[512] = ""; }
using cs::fail;
using cs::NttPlan;
using cs::CosetTable;
using cs::PeriodicTable;
using cs::g_err;

namespace {

// frees the device allocations registered with it unless release() is reached: error paths of the table builders leak nothing
struct DevGuard {
    std::vector<void *> ptrs;
    bool armed = true;
    template <class T> hipError_t alloc(T **p, size_t bytes) {
        const hipError_t e = hipMalloc((void **)p, bytes);
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    void release() { armed = false; }
    ~DevGuard() { if (armed) for (void *q : ptrs) (void)hipFree(q); }
};

// The fixed-base table of the signing calls (trace_gen.h: 990 multiples of G, constants only), one per context: built on the context's
// stream by its first signing call, found again by the context's address, freed by cstark_ctx_destroy.  It is kept beside struct
// cstark_ctx, not in it: it is no function of anything a call passes in, so no call history can change what it holds.
std::mutex &g_sign_tables_lock = *new std::mutex; // never destroyed: a context may be destroyed while the process exits
std::unordered_map<const cstark_ctx *, uint64_t *> &g_sign_tables = *new std::unordered_map<const cstark_ctx *, uint64_t *>;
uint64_t *sign_table_find(const cstark_ctx *c) {
    std::lock_guard<std::mutex> hold(g_sign_tables_lock);
    const auto it = g_sign_tables.find(c);
    return it == g_sign_tables.end() ? nullptr : it->second;
}
void sign_table_keep(const cstark_ctx *c, uint64_t *table) {
    std::lock_guard<std::mutex> hold(g_sign_tables_lock);
    g_sign_tables[c] = table;
}
void sign_table_release(const cstark_ctx *c) {
    std::lock_guard<std::mutex> hold(g_sign_tables_lock);
    const auto it = g_sign_tables.find(c);
    if (it == g_sign_tables.end()) return;
    (void)hipFree(it->second);
    g_sign_tables.erase(it);
}

// The proof form of the contexts that were set to another than CSTARK_FORM_PLAIN (cstark_ctx_set_proof_form), by the context's address
// like the table above; the entry goes with the context.  One word that only its setter writes: no prover, verifier or ledger call
// reads or changes anything else by it, and no call but the setter changes it.
std::unordered_map<const cstark_ctx *, uint32_t> &g_proof_forms = *new std::unordered_map<const cstark_ctx *, uint32_t>;
void proof_form_release(const cstark_ctx *c) {
    std::lock_guard<std::mutex> hold(g_sign_tables_lock);
    g_proof_forms.erase(c);
}

int get_plan(cstark_ctx *c, unsigned log_n, const NttPlan **out) {
    for (const NttPlan &p : c->plans)
        if (p.log_n == log_n) { *out = &p; return CSTARK_OK; }
    const size_t n = (size_t)1 << log_n;
    NttPlan p{log_n, nullptr, nullptr, 0};
    DevGuard g;
    HIP_TRY(g.alloc(&p.w, n * 8));
    HIP_TRY(g.alloc(&p.winv, n * 8));
    const uint64_t w = cs::host::root_of_unity(log_n);
    HIP_TRY(cs::ntt_power_table(p.w, n, w, c->stream));
    HIP_TRY(cs::ntt_power_table(p.winv, n, cs::host::inv(w), c->stream));
    p.n_inv = cs::host::inv(cs::host::from_u64(n));
    cs::NttThreeStepShape shape;
    if (cs::ntt_three_step_shape(log_n, &shape)) { // here and in get_coset_table: the dense tables ntt_columns requires at exactly these sizes
        const size_t words = cs::ntt_aux_plan_words(shape);
        HIP_TRY(g.alloc(&p.aux_w, words * 8));
        HIP_TRY(g.alloc(&p.aux_winv, words * 8));
        HIP_TRY(cs::ntt_build_aux_plan(p.aux_w, p.w, shape, c->stream));
        HIP_TRY(cs::ntt_build_aux_plan(p.aux_winv, p.winv, shape, c->stream));
    }
    c->plans.push_back(p);
    g.release();
    *out = &c->plans.back();
    return CSTARK_OK;
}

int get_coset_table(cstark_ctx *c, unsigned log_n, unsigned log_b, uint64_t offset, const CosetTable **out) {
    for (const CosetTable &t : c->cosets)
        if (t.log_n == log_n && t.log_b == log_b && t.offset == offset) { *out = &t; return CSTARK_OK; }
    const size_t n = (size_t)1 << log_n, b = (size_t)1 << log_b;
    CosetTable t{log_n, log_b, offset, nullptr};
    DevGuard g;
    HIP_TRY(g.alloc(&t.s, b * n * 8));
    const uint64_t wbn = cs::host::root_of_unity(log_n + log_b);
    uint64_t shift = offset;
    for (size_t k = 0; k < b; k++) {
        HIP_TRY(cs::ntt_power_table(t.s + k * n, n, shift, c->stream));
        shift = cs::host::mul(shift, wbn);
    }
    cs::NttThreeStepShape shape;
    if (cs::ntt_three_step_shape(log_n, &shape)) {
        const NttPlan *p;
        RC_TRY(get_plan(c, log_n, &p));
        t.aux_words = cs::ntt_aux_coset_words(shape);
        HIP_TRY(g.alloc(&t.aux, b * t.aux_words * 8));
        for (size_t k = 0; k < b; k++) HIP_TRY(cs::ntt_build_aux_coset(t.aux + k * t.aux_words, p->w, t.s + k * n, shape, c->stream));
    }
    c->cosets.push_back(t);
    g.release();
    *out = &c->cosets.back();
    return CSTARK_OK;
}

int ensure_ws(cstark_ctx *c, size_t bytes) {
    if (bytes <= c->ws_bytes) return CSTARK_OK;
    if (c->ws) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
    HIP_TRY(hipMalloc(&c->ws, bytes));
    c->ws_bytes = bytes;
    return CSTARK_OK;
}

} // namespace
uint32_t cs::ctx_proof_form(const cstark_ctx *c) {
    std::lock_guard<std::mutex> hold(g_sign_tables_lock);
    const auto it = g_proof_forms.find(c);
    return it == g_proof_forms.end() ? (uint32_t)CSTARK_FORM_PLAIN : it->second;
}
int plan_tables(cstark_ctx *c, unsigned log_n, const uint64_t **w, const uint64_t **winv) {
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    *w = p->w; *winv = p->winv;
    return CSTARK_OK;
}
namespace {

int interpolate_impl(cstark_ctx *c, uint64_t *d_evals, uint64_t *d_coeffs, uint32_t width, uint32_t log_n) {
    if (!c || !d_evals || !d_coeffs || width == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_interpolate_columns: bad argument");
    if (d_evals == d_coeffs) return fail(CSTARK_ERR_INVALID_ARG, "cstark_interpolate_columns: output must not alias input");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "domain size must be 2^6 .. 2^24");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    cs::NttArgs a{};
    a.in = d_evals; a.scratch = d_evals; a.out = d_coeffs;
    a.width = width; a.batch = 1; a.log_n = log_n;
    a.w = p->winv; a.post_scale = p->n_inv; a.do_scale = true; a.inverse = true; a.aux = p->aux_winv;
    HIP_TRY(cs::ntt_columns(a, c->stream));
    return CSTARK_OK;
}

// part timing: an event on the stream, from a pool that grows on demand up to LDE_EVENT_CAP (reset by cstark_lde_timing_ms; a caller
// that never collects stops being timed instead of growing the pool without bound)
constexpr size_t LDE_EVENT_CAP = 4096;
int lde_mark(cstark_ctx *c) {
    if (c->lde_ev_used == c->lde_ev.size()) {
        if (c->lde_ev.size() >= LDE_EVENT_CAP) return CSTARK_ERR_UNSUPPORTED; // pool full: this extension is not timed

        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->lde_ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(c->lde_ev[c->lde_ev_used++], c->stream));
    return CSTARK_OK;
}

// All cosets of an extension go into ONE launch pair (the grid's batch dimension) when their intermediate fits this budget: the eight
// cosets of a coefficient tile then run together on one XCD and the coefficients are read from HBM once (ntt.hip, k_ntt_cols_v5).  7 GiB
// covers the 94 x 2^20 x 8 trace (6.3 GB; HBM holds 288 GB); CSTARK_LDE_BATCH_MB overrides (tuning; 0 = coset by coset as in round 2).
// (clamped to 0 .. 64 GiB: a negative or absurd value must not become a huge size_t).  Footprint: the workspace of a context grows to the
// largest batch it has extended -- 6.3 GB for the 94 x 2^20 x 8 trace -- and stays: every context (ProverPool worker, shard rank) holds
// its own.  If that allocation fails the extension falls back to one coset at a time (0.8 GB).
const size_t LDE_BATCH_WS_BYTES = [] {
    const char *e = getenv("CSTARK_LDE_BATCH_MB");
    if (!e) return (size_t)7 << 30;
    const long long mb = atoll(e);
    return mb <= 0 ? (size_t)0 : mb > (64ll << 10) ? (size_t)64 << 30 : (size_t)mb << 20;
}();
int lde_impl_inner(cstark_ctx *c, const uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols, uint32_t log_n,
                   uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk);
// one extension of `units` elements between an event pair of the part timing
template <class F>
int lde_timed(cstark_ctx *c, uint64_t units, F &&run) {
    // events come in pairs: without room for both, or if the first cannot be recorded, the extension simply is not timed
    bool timed = c && c->part_timing && c->lde_ev_used + 2 <= LDE_EVENT_CAP;
    const size_t mark = timed ? c->lde_ev_used : 0;
    if (timed && lde_mark(c) != CSTARK_OK) { c->lde_ev_used = mark; timed = false; }
    const int rc = run();
    if (timed) {
        if (rc == CSTARK_OK && lde_mark(c) == CSTARK_OK) c->lde_units += units;
        else c->lde_ev_used = mark; // never leave an unpaired event behind
    }
    return rc;
}
int lde_impl(cstark_ctx *c, const uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols, uint32_t log_n, uint32_t log_blowup,
             uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    return lde_timed(c, (uint64_t)ncols * nk << log_n, [&] { return lde_impl_inner(c, d_coeffs, d_lde, width, col0, ncols, log_n, log_blowup, domain_offset, k0, nk); });
}
int lde_impl_inner(cstark_ctx *c, const uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols, uint32_t log_n,
                   uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    if (!c || !d_coeffs || !d_lde || width == 0 || ncols == 0 || (uint64_t)col0 + ncols > width) return fail(CSTARK_ERR_INVALID_ARG, "cstark_lde_columns: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6) return fail(CSTARK_ERR_UNSUPPORTED, "unsupported domain size");
    if (domain_offset == 0 || domain_offset >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "domain offset must be a nonzero field element");
    if ((uint64_t)k0 + nk > (1ull << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "coset range exceeds the blowup factor");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    const CosetTable *t;
    RC_TRY(get_plan(c, log_n, &p));
    RC_TRY(get_coset_table(c, log_n, log_blowup, domain_offset, &t));
    const size_t n = (size_t)1 << log_n;
    RC_TRY(ensure_ws(c, (size_t)width * n * 8));
    // Measured on MI355X at 2^20 x 94 x 8 and dropped: column groups with the cosets inside, so that a group's coefficients and the
    // intermediate of the two-pass transform stay within the 256 MB Infinity Cache -- all columns at once 10.33 ms, groups of 32 / 16 /
    // 8 / 4 columns 10.49 / 10.80 / 11.13 / 12.17 ms: the transform is bound by its field multiplications, not by HBM.
    cs::NttArgs a{};
    a.in = d_coeffs + (size_t)col0 * n; a.scratch = (uint64_t *)c->ws;
    a.width = ncols; a.log_n = log_n;
    a.w = p->w; a.do_scale = false; a.aux = p->aux_w;
    // all cosets in one launch pair -- the grid's batch dimension -- when the intermediate of every coset fits the workspace budget:
    // 2 launches of nk x the workgroups instead of 2 nk small ones
    if (nk > 1 && (size_t)nk * ncols * n * 8 <= LDE_BATCH_WS_BYTES) {
        if (ensure_ws(c, (size_t)nk * ncols * n * 8) == CSTARK_OK) {
            a.scratch = (uint64_t *)c->ws; a.out = d_lde + (size_t)col0 * n; a.batch = nk;
            a.prescale = t->s + (size_t)k0 * n; a.prescale_batch_stride = n;
            a.aux_ps = t->aux ? t->aux + (size_t)k0 * t->aux_words : nullptr; a.aux_ps_batch_stride = t->aux_words;
            a.in_batch_stride = 0; a.scratch_batch_stride = (size_t)ncols * n; a.out_batch_stride = (size_t)width * n;
            HIP_TRY(cs::ntt_columns(a, c->stream));
            return CSTARK_OK;
        }
        (void)hipGetLastError(); // no room for the batched intermediate: coset by coset
        RC_TRY(ensure_ws(c, (size_t)width * n * 8));
        a.scratch = (uint64_t *)c->ws;
    }
    a.batch = 1;
    for (uint32_t k = k0; k < k0 + nk; k++) {
        a.out = d_lde + ((size_t)(k - k0) * width + col0) * n;
        a.prescale = t->s + (size_t)k * n;
        a.aux_ps = t->aux ? t->aux + (size_t)k * t->aux_words : nullptr;
        HIP_TRY(cs::ntt_columns(a, c->stream));
    }
    return CSTARK_OK;
}

// Step columns (ntt.h): the constants of one (trace length, blowup, offset, block length) -- D and, per coset, the column pass of D.
// Built on first use on the context's stream, freed with the context; 8 (1 + b) n bytes: 72 MB at 2^20 rows and blowup 8.
// split = R > 0: the same for D_R, the second pair of tables of the two-level columns.
int get_step_table(cstark_ctx *c, unsigned log_n, unsigned log_b, uint64_t offset, unsigned log_block, unsigned split, const cs::StepTable **out) {
    for (const cs::StepTable &t : c->steps)
        if (t.log_n == log_n && t.log_b == log_b && t.offset == offset && t.log_block == log_block && t.split == split) { *out = &t; return CSTARK_OK; }
    const NttPlan *p;
    const CosetTable *ct;
    RC_TRY(get_plan(c, log_n, &p));
    RC_TRY(get_coset_table(c, log_n, log_b, offset, &ct));
    const size_t n = (size_t)1 << log_n, b = (size_t)1 << log_b;
    cs::StepTable t{log_n, log_b, offset, log_block, split, nullptr, nullptr};
    DevGuard g;
    HIP_TRY(g.alloc(&t.d, n * 8));
    HIP_TRY(g.alloc(&t.w, b * n * 8));
    cs::NttArgs a{};
    a.in = t.d; a.scratch = t.w; a.width = 1; a.batch = (unsigned)b; a.log_n = log_n;
    a.w = p->w; a.aux = p->aux_w;
    a.prescale = ct->s; a.prescale_batch_stride = n;
    a.aux_ps = ct->aux; a.aux_ps_batch_stride = ct->aux_words;
    a.in_batch_stride = 0; a.scratch_batch_stride = n;
    HIP_TRY(cs::ntt_step_build_tables(t.d, log_block, split, p->winv, a, c->stream));
    c->steps.push_back(t);
    g.release();
    *out = &c->steps.back();
    return CSTARK_OK;
}
// Coefficients and extension of columns [col0, col0 + ncols) that are constant over blocks of block_len rows.  Where the transform serves
// the shape (cs::ntt_step_shape) only the first row of every block is read and d_evals stays intact; everywhere else the columns take
// interpolate_impl (which destroys them) and lde_impl.
// split = R > 0: two-level columns, one value on rows [0, R) of every block and another on rows [R, block_len); rows 0 and R are read.
int step_impl(cstark_ctx *c, uint64_t *d_evals, uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols, uint32_t log_n,
              uint32_t block_len, uint32_t split, uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    if (!c || !d_evals || !d_coeffs || !d_lde || width == 0 || ncols == 0 || (uint64_t)col0 + ncols > width)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_step_columns: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6) return fail(CSTARK_ERR_UNSUPPORTED, "unsupported domain size");
    if (block_len == 0 || (block_len & (block_len - 1)) || block_len > (1u << log_n)) return fail(CSTARK_ERR_INVALID_ARG, "the block length must be a power of two up to the trace length");
    if (split >= block_len) return fail(CSTARK_ERR_INVALID_ARG, "the split row must lie inside the block");
    if (domain_offset == 0 || domain_offset >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "domain offset must be a nonzero field element");
    if ((uint64_t)k0 + nk > (1ull << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "coset range exceeds the blowup factor");
    const size_t n = (size_t)1 << log_n;
    const unsigned log_block = (unsigned)__builtin_ctz(block_len);
    if (!cs::ntt_step_shape(log_n, log_block)) {
        RC_TRY(interpolate_impl(c, d_evals + (size_t)col0 * n, d_coeffs + (size_t)col0 * n, ncols, log_n));
        return lde_impl(c, d_coeffs, d_lde, width, col0, ncols, log_n, log_blowup, domain_offset, k0, nk);
    }
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    const cs::StepTable *t;
    RC_TRY(get_plan(c, log_n, &p));
    const cs::StepTable *tr = nullptr;
    RC_TRY(get_step_table(c, log_n, log_blowup, domain_offset, log_block, 0, &t));
    if (split) RC_TRY(get_step_table(c, log_n, log_blowup, domain_offset, log_block, split, &tr));
    RC_TRY(ensure_ws(c, ((size_t)ncols << (log_n - log_block)) * (split ? 16 : 8))); // the factors A [ncols][T], or A1 | A2 [ncols][2][T]
    uint64_t *fac = (uint64_t *)c->ws;
    if (split)
        HIP_TRY(cs::ntt_step2_coefficients(d_evals + (size_t)col0 * n, fac, d_coeffs + (size_t)col0 * n, t->d, tr->d, ncols, log_n, log_block, split, p->winv,
                                           p->n_inv, c->stream));
    else
        HIP_TRY(cs::ntt_step_coefficients(d_evals + (size_t)col0 * n, fac, d_coeffs + (size_t)col0 * n, t->d, ncols, log_n, log_block, p->winv, p->n_inv, c->stream));
    return lde_timed(c, (uint64_t)ncols * nk << log_n, [&] {
        cs::NttArgs a{};
        a.out = d_lde + (size_t)col0 * n; a.width = ncols; a.batch = nk; a.log_n = log_n;
        a.out_batch_stride = (size_t)width * n; a.aux = p->aux_w;
        HIP_TRY(cs::ntt_step_rows(a, t->w + (size_t)k0 * n, tr ? tr->w + (size_t)k0 * n : nullptr, fac, log_block, c->stream));
        return (int)CSTARK_OK;
    });
}

// Periodic columns over the LDE domain: host columns [ncols][2^log_cycle] -> *d_tab = [b][ncols][cycle], an allocation of `keep`.  A
// column of period `cycle` is a polynomial of degree < cycle in x^(n/cycle): interpolated over the cycle, then evaluated over
// offset' * <w_{b*cycle}>, offset' = g^(n/cycle).  Returns with the stream idle: `cols` may go out of scope, the scratch is freed.
int extend_periodic_columns(cstark_ctx *c, const std::vector<uint64_t> &cols, uint32_t ncols, uint32_t log_cycle, unsigned log_n, unsigned log_b,
                            DevGuard &keep, uint64_t **d_tab) {
    const size_t words = (size_t)ncols << log_cycle, n = (size_t)1 << log_n;
    uint64_t *d_cols = nullptr, *d_poly = nullptr;
    DevGuard tmp; // never released: frees the scratch on every path
    HIP_TRY(tmp.alloc(&d_cols, words * 8));
    HIP_TRY(tmp.alloc(&d_poly, words * 8));
    HIP_TRY(keep.alloc(d_tab, (words << log_b) * 8));
    HIP_TRY(hipMemcpyAsync(d_cols, cols.data(), words * 8, hipMemcpyHostToDevice, c->stream));
    RC_TRY(interpolate_impl(c, d_cols, d_poly, ncols, log_cycle));
    RC_TRY(lde_impl(c, d_poly, *d_tab, ncols, 0, ncols, log_cycle, log_b, cs::host::pow(cs::host::lde_offset(), n >> log_cycle), 0, 1u << log_b));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CSTARK_OK;
}

// K7: periodic values of the 48 mask / round-constant columns over the constraint-evaluation domain, plus the
// per-coset scalars of the driver.  Built once per (depth, trace length, blowup) and cached.
int get_periodic(cstark_ctx *c, unsigned depth, unsigned log_n, unsigned log_b, const PeriodicTable **out) {
    for (const PeriodicTable &t : c->periodic)
        if (t.depth == depth && t.log_n == log_n && t.log_b == log_b) { *out = &t; return CSTARK_OK; }
    if (log_n < 10) return fail(CSTARK_ERR_INVALID_ARG, "the trace must hold at least one 1024-row transaction");
    std::vector<uint64_t> cols;
    if (!cs::host::tx_periodic_columns(depth, cols)) return fail(CSTARK_ERR_INVALID_ARG, "unsupported Merkle depth");
    static_assert(cs::host::TX_CYCLE == 1 << 10, "the cycle of TransactionAir's periodic columns");
    const size_t n = (size_t)1 << log_n, b = (size_t)1 << log_b;
    PeriodicTable t{depth, log_n, log_b, nullptr, nullptr, nullptr};
    DevGuard keep;
    RC_TRY(extend_periodic_columns(c, cols, cs::host::TX_NUM_PERIODIC, 10, log_n, log_b, keep, &t.tab));
    HIP_TRY(keep.alloc(&t.coset, b * cs::CE_COSET_CONSTS * 8));
    const uint64_t g = cs::host::lde_offset();
    // per-coset scalars: shift_k = g w_{bn}^k, 1/(shift^n - 1), shift^adj_g, shift^badj
    std::vector<uint64_t> cc(b * cs::CE_COSET_CONSTS);
    const uint64_t wbn = cs::host::root_of_unity(log_n + log_b);
    uint64_t shift = g;
    for (size_t k = 0; k < b; k++) {
        uint64_t *o = cc.data() + k * cs::CE_COSET_CONSTS;
        o[0] = shift;
        o[1] = cs::host::inv(cs::host::sub(cs::host::pow(shift, n), cs::host::ONE));
        for (int gi = 0; gi < 5; gi++) o[2 + gi] = cs::host::pow(shift, cs::host::tx_group_adjustment(gi, n, n * b));
        o[7] = cs::host::pow(shift, cs::host::tx_boundary_adjustment(n, n * b));
        o[8] = cs::host::pow(shift, n - 1); // lift between neighbouring degree groups (merged split polynomials)
        o[9] = 0;
        shift = cs::host::mul(shift, wbn);
    }
    HIP_TRY(hipMemcpyAsync(t.coset, cc.data(), cc.size() * 8, hipMemcpyHostToDevice, c->stream));
    const NttPlan *plan;
    RC_TRY(get_plan(c, log_n, &plan));
    HIP_TRY(keep.alloc(&t.binv, b * 2 * n * 8));
    HIP_TRY(cs::build_boundary_inverses(t.binv, plan->w, t.coset, cs::host::inv(cs::host::root_of_unity(log_n)), log_n, log_b, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // cc goes out of scope
    keep.release();
    c->periodic.push_back(t);
    *out = &c->periodic.back();
    return CSTARK_OK;
}

// The standalone sub-AIRs' periodic columns over the LDE domain, built once per (AIR, depth, trace length, blowup): MerkleAir
// [b][33][512] (depth: its hash length), SchnorrAir [b][36][512], RescueAir [b][29][8] (both: depth 0)
int get_small_periodic(cstark_ctx *c, int air, unsigned depth, unsigned log_n, unsigned log_b, const PeriodicTable **out) {
    for (const PeriodicTable &t : c->small_periodic)
        if (t.air == air && t.depth == depth && t.log_n == log_n && t.log_b == log_b) { *out = &t; return CSTARK_OK; }
    PeriodicTable t{depth, log_n, log_b, nullptr, nullptr, nullptr, air};
    std::vector<uint64_t> cols;
    DevGuard keep;
    if (air == CSTARK_AIR_MERKLE_UPDATE) {
        if (!cs::host::merkle_periodic_columns(depth, cols)) return fail(CSTARK_ERR_INVALID_ARG, "unsupported Merkle depth");
        RC_TRY(extend_periodic_columns(c, cols, 33, 9, log_n, log_b, keep, &t.tab));
    } else if (air == CSTARK_AIR_SCHNORR) {
        cs::host::schnorr_mask_columns(cols);
        RC_TRY(extend_periodic_columns(c, cols, 36, 9, log_n, log_b, keep, &t.tab));
    } else if (air == CSTARK_AIR_RESCUE_CHAIN) {
        // 8 x 29 x b values, computed on the host: the transform kernels start at 64 points
        using namespace cs::host;
        rescue_chain_periodic_columns(cols);
        const size_t n = (size_t)1 << log_n, b = (size_t)1 << log_b;
        for (int cidx = 0; cidx < 29; cidx++) intt_small(cols.data() + (size_t)cidx * 8, 3);
        std::vector<uint64_t> tab(b * 29 * 8);
        const uint64_t wbn = root_of_unity(log_n + log_b), w8 = root_of_unity(3);
        uint64_t shift = lde_offset();
        for (size_t k = 0; k < b; k++) {
            uint64_t x = pow(shift, n / 8); // point m of coset k in the variable x^(n/8): shift^(n/8) w_8^m
            for (int m = 0; m < 8; m++) {
                for (int cidx = 0; cidx < 29; cidx++) {
                    const uint64_t *co = cols.data() + (size_t)cidx * 8;
                    uint64_t v = 0;
                    for (int d = 7; d >= 0; d--) v = add(mul(v, x), co[d]);
                    tab[(k * 29 + cidx) * 8 + m] = v;
                }
                x = mul(x, w8);
            }
            shift = mul(shift, wbn);
        }
        HIP_TRY(keep.alloc(&t.tab, tab.size() * 8));
        HIP_TRY(hipMemcpyAsync(t.tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        return fail(CSTARK_ERR_UNSUPPORTED, "AIR not available through the generic entry points");
    }
    keep.release();
    c->small_periodic.push_back(t);
    *out = &c->small_periodic.back();
    return CSTARK_OK;
}

// The matrix of the generator addition on the doubling's six products (generator_fold.h), derived on the host and uploaded once per
// context: a constant of the curve, read by the per-proof fold of the composition coefficients (constraints.hip)
int generator_fold_table(cstark_ctx *c, const uint64_t **d_j) {
    static_assert(cs::hostg::GF_COMPONENTS == cs::CE_GFOLD_COMPONENTS && cs::hostg::GF_LAMBDA_WORDS == cs::CE_GFOLD_WORDS &&
                  cs::hostg::GF_OUTPUTS * cs::hostg::GF_COMPONENTS == cs::CE_GFOLD_J_WORDS, "generator fold layout");
    if (!c->gfold_j) {
        std::vector<uint64_t> j(cs::CE_GFOLD_J_WORDS);
        cs::hostg::generator_fold_matrix(j.data());
        DevGuard keep;
        uint64_t *d = nullptr;
        HIP_TRY(keep.alloc(&d, j.size() * 8));
        HIP_TRY(hipMemcpyAsync(d, j.data(), j.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        keep.release();
        c->gfold_j = d;
    }
    *d_j = c->gfold_j;
    return CSTARK_OK;
}

int ce_params(cstark_ctx *c, const uint64_t *d_lde, uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n, uint32_t log_blowup, uint32_t k0,
              uint32_t nk, cs::CeParams *p) {
    if (!c || !d_lde || !d_out) return fail(CSTARK_ERR_INVALID_ARG, "constraint evaluation: null argument");
    if (((uintptr_t)d_lde & 15) != 0) return fail(CSTARK_ERR_INVALID_ARG, "constraint evaluation: d_lde must be 16-byte aligned (16-byte LDS-DMA pieces)");
    if (log_n < 10 || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_INVALID_ARG, "trace length must be 2^10 .. 2^24");
    if (log_blowup != 3) return fail(CSTARK_ERR_UNSUPPORTED, "TransactionAir needs a constraint-evaluation blowup of 8 (max degree 7, src/air.rs:76-108)");
    if ((uint64_t)k0 + nk > (1ull << log_blowup) || nk == 0) return fail(CSTARK_ERR_INVALID_ARG, "coset range exceeds the blowup factor");
    HIP_TRY(hipSetDevice(c->device));
    const PeriodicTable *pt;
    const NttPlan *plan;
    RC_TRY(get_periodic(c, merkle_depth, log_n, log_blowup, &pt));
    RC_TRY(get_plan(c, log_n, &plan));
    const uint64_t n = 1ull << log_n, ce = n << log_blowup;
    *p = cs::CeParams{};
    p->lde = d_lde; p->ptab = pt->tab; p->w = plan->w; p->coset = pt->coset; p->binv = pt->binv; p->out = d_out;
    p->w_last = cs::host::inv(cs::host::root_of_unity(log_n));
    for (int g = 0; g < 5; g++) p->adj_mod_n[g] = (uint32_t)(cs::host::tx_group_adjustment(g, n, ce) & (n - 1));
    p->badj_mod_n = (uint32_t)(cs::host::tx_boundary_adjustment(n, ce) & (n - 1));
    p->log_n = log_n; p->log_b = log_blowup; p->k0 = k0;
    RC_TRY(generator_fold_table(c, &p->gfold_j));
    return CSTARK_OK;
}

} // namespace

// the resident witness allocation of n transfers at depth d (witness_layout.h: one allocation, 8-byte fields first), grown when needed
int tx_witness_reserve(cstark_ctx *c, size_t n, size_t d, size_t *sz, size_t *off) {
    cs::witness_segments(n, d, sz, off);
    const size_t total = off[cs::WIT_NUM_SEGMENTS];
    if (total > c->wit_bytes) {
        if (c->wit_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->wit_buf)); c->wit_buf = nullptr; c->wit_bytes = 0; }
        HIP_TRY(hipMalloc(&c->wit_buf, total));
        c->wit_bytes = total;
    }
    return CSTARK_OK;
}
// ... and the context's view of it, once its segments are written (or enqueued on the context's stream)
void tx_witness_bind(cstark_ctx *c, size_t n, size_t d, const size_t *off) {
    char *base = (char *)c->wit_buf;
    cs::TxWitnessDev &dv = c->wit;
    dv.n_tx = (uint32_t)n;
    dv.depth = (uint32_t)d;
    dv.initial_roots = (const uint64_t *)(base + off[cs::WIT_INITIAL_ROOTS]);
    dv.s_old = (const uint64_t *)(base + off[cs::WIT_S_OLD]);
    dv.r_old = (const uint64_t *)(base + off[cs::WIT_R_OLD]);
    dv.s_idx = (const uint64_t *)(base + off[cs::WIT_S_IDX]);
    dv.r_idx = (const uint64_t *)(base + off[cs::WIT_R_IDX]);
    dv.s_paths = (const uint64_t *)(base + off[cs::WIT_S_PATHS]);
    dv.r_paths = (const uint64_t *)(base + off[cs::WIT_R_PATHS]);
    dv.deltas = (const uint64_t *)(base + off[cs::WIT_DELTAS]);
    dv.sig_rx = (const uint64_t *)(base + off[cs::WIT_SIG_RX]);
    dv.h_limbs = (uint64_t *)(base + off[cs::WIT_H_LIMBS]);
    dv.sig_s = (const uint8_t *)(base + off[cs::WIT_SIG_S]);
    dv.msg_tail = nullptr;
}

extern "C" {

const char *cstark_last_error(void) { return g_err; }
const char *cstark_version(void) { return "certificate-stark_amd 0.2 (gfx950)"; }

int cstark_ctx_create(int device, void *stream, cstark_ctx **out) {
    if (!out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ctx_create: out is null");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(CSTARK_ERR_NO_DEVICE, "no HIP device visible (this backend has no CPU fallback)");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= count) return fail(CSTARK_ERR_INVALID_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    cstark_ctx *c = new (std::nothrow) cstark_ctx();
    if (!c) return fail(CSTARK_ERR_OOM, "host allocation failed");
    c->device = device;
    c->stream = (hipStream_t)stream; // NULL is HIP's default stream
    // the internal streams carry latency-bound recurrences (one wave per transaction and chain) that run beside chip-filling
    // transforms on the caller's stream: highest dispatch priority, so that their workgroups are placed as soon as they are ready
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&c->side2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_mid, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return fail(CSTARK_ERR_HIP, "could not create the internal stream / events");
    }
    *out = c;
    return CSTARK_OK;
}
int cstark_ctx_create_own_stream(int device, cstark_ctx **out) {
    if (!out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ctx_create_own_stream: out is null");
    RC_TRY(cstark_ctx_create(device, nullptr, out));
    cstark_ctx *c = *out;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->stream = nullptr;
        cstark_ctx_destroy(c);
        *out = nullptr;
        return fail(CSTARK_ERR_HIP, "could not create the context's stream");
    }
    c->owns_stream = true;
    return CSTARK_OK;
}

void cstark_ctx_destroy(cstark_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if (c->side2) { (void)hipStreamSynchronize(c->side2); (void)hipStreamDestroy(c->side2); }
    if (c->ev_join2) (void)hipEventDestroy(c->ev_join2);
    if (c->ev_mid) (void)hipEventDestroy(c->ev_mid);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->wit_buf) (void)hipFree(c->wit_buf);
    if (c->ws) (void)hipFree(c->ws);
    if (c->coef_buf) (void)hipFree(c->coef_buf);
    if (c->gfold_j) (void)hipFree(c->gfold_j);
    if (c->coef_stage) (void)hipHostFree(c->coef_stage);
    if (c->coef_ev) (void)hipEventDestroy(c->coef_ev);
    for (NttPlan &p : c->plans) { (void)hipFree(p.w); (void)hipFree(p.winv); (void)hipFree(p.aux_w); (void)hipFree(p.aux_winv); }
    for (CosetTable &t : c->cosets) { (void)hipFree(t.s); (void)hipFree(t.aux); }
    for (cs::StepTable &t : c->steps) { (void)hipFree(t.d); (void)hipFree(t.w); }
    for (PeriodicTable &t : c->periodic) { (void)hipFree(t.tab); (void)hipFree(t.coset); (void)hipFree(t.binv); }
    for (PeriodicTable &t : c->small_periodic) (void)hipFree(t.tab);
    for (cs::AssertInverseTable &t : c->assert_inv) (void)hipFree(t.tab);
    for (cs::AirCombineStatic &t : c->air_static) (void)hipFree(t.d_static);
    if (c->air_coef_buf) (void)hipFree(c->air_coef_buf);
    if (c->air_coef_stage) (void)hipHostFree(c->air_coef_stage);
    if (c->air_coef_ev) (void)hipEventDestroy(c->air_coef_ev);
    if (c->deep_buf) (void)hipFree(c->deep_buf);
    if (c->deep_stage) (void)hipHostFree(c->deep_stage);
    if (c->deep_ev) (void)hipEventDestroy(c->deep_ev);
    if (c->desc_buf) (void)hipFree(c->desc_buf);
    if (c->rb_dev) (void)hipFree(c->rb_dev);
    if (c->shard_bit37) (void)hipFree(c->shard_bit37);
    if (c->rb_host) (void)hipHostFree(c->rb_host);
    if (c->tail_buf) (void)hipFree(c->tail_buf);
    if (c->sig_buf) (void)hipFree(c->sig_buf);
    sign_table_release(c);
    proof_form_release(c);
    if (c->path_buf) (void)hipFree(c->path_buf);
    if (c->multi_buf) (void)hipFree(c->multi_buf);
    witness_check_release(c);
    for (cs::RawPeriodic &t : c->raw_periodic) (void)hipFree(t.tab);
    if (c->val_buf) (void)hipFree(c->val_buf);
    if (c->arena) cs::prove_arena_free(c->arena);
    if (c->verify) cs::verify_arena_free(c->verify);
    for (hipEvent_t e : c->part_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->lde_ev) (void)hipEventDestroy(e);
    if (c->owns_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int cstark_ctx_set_proof_form(cstark_ctx *c, uint32_t form) {
    if (!c) return fail(CSTARK_ERR_INVALID_ARG, "null context");
    if (form != CSTARK_FORM_PLAIN && form != CSTARK_FORM_COMPACT) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ctx_set_proof_form: CSTARK_FORM_PLAIN or CSTARK_FORM_COMPACT");
    std::lock_guard<std::mutex> hold(g_sign_tables_lock);
    if (form == CSTARK_FORM_PLAIN) g_proof_forms.erase(c);
    else g_proof_forms[c] = form;
    return CSTARK_OK;
}
int cstark_ctx_proof_form(cstark_ctx *c, uint32_t *form) {
    if (!c || !form) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    *form = cs::ctx_proof_form(c);
    return CSTARK_OK;
}

int cstark_ctx_synchronize(cstark_ctx *c) {
    if (!c) return fail(CSTARK_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CSTARK_OK;
}

int cstark_malloc(cstark_ctx *c, size_t bytes, void **d_ptr) {
    if (!c || !d_ptr) return fail(CSTARK_ERR_INVALID_ARG, "cstark_malloc: null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return CSTARK_OK;
}
int cstark_free(cstark_ctx *c, void *d_ptr) {
    if (!c) return fail(CSTARK_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(d_ptr));
    return CSTARK_OK;
}
int cstark_memcpy_h2d(cstark_ctx *c, void *d_dst, const void *src, size_t bytes) {
    if (!c || (!d_dst && bytes) || (!src && bytes)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_memcpy_h2d: null argument");
    HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CSTARK_OK;
}
int cstark_memcpy_d2h(cstark_ctx *c, void *dst, const void *d_src, size_t bytes) {
    if (!c || (!dst && bytes) || (!d_src && bytes)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_memcpy_d2h: null argument");
    HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CSTARK_OK;
}

// ---- K1 ------------------------------------------------------------------------------------------
int cstark_tx_witness_upload(cstark_ctx *c, const cstark_tx_witness *w) {
    if (!c || !w) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_witness_upload: null argument");
    const size_t n = w->n_tx, d = w->merkle_depth;
    if (n == 0) return fail(CSTARK_ERR_INVALID_ARG, "n_tx must be positive");
    // (depth+1) must be a power of two (src/lib.rs:102-105) and 8*depth+7 <= 511 rows (src/merkle/constants.rs:27-29)
    if (d == 0 || ((d + 1) & d) != 0 || 8 * d + 7 > 511) return fail(CSTARK_ERR_INVALID_ARG, "tree depth must be one less than a power of 2 and at most 31");
    if (!w->initial_roots || !w->s_old_values || !w->r_old_values || !w->s_indices || !w->r_indices || !w->s_paths || !w->r_paths ||
        !w->deltas || !w->sig_rx || !w->sig_s)
        return fail(CSTARK_ERR_INVALID_ARG, "witness array pointer is null");
    HIP_TRY(hipSetDevice(c->device));
    const void *src[] = {w->initial_roots, w->s_old_values, w->r_old_values, w->s_indices, w->r_indices, w->s_paths, w->r_paths, w->deltas, w->sig_rx, nullptr, w->sig_s};
    size_t sz[cs::WIT_NUM_SEGMENTS], off[cs::WIT_NUM_SEGMENTS + 1];
    RC_TRY(tx_witness_reserve(c, n, d, sz, off));
    char *base = (char *)c->wit_buf;
    for (int i = 0; i < cs::WIT_NUM_SEGMENTS; i++)
        if (src[i]) HIP_TRY(hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the caller may free its host arrays on return
    tx_witness_bind(c, n, d, off);
    return CSTARK_OK;
}

int cstark_tx_build_trace(cstark_ctx *c, uint64_t *d_trace) {
    if (!c || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_build_trace: null argument");
    if (!c->wit_buf || c->wit.n_tx == 0) return fail(CSTARK_ERR_INVALID_ARG, "no witness uploaded");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_trace_gen(c->wit, d_trace, c->stream, c->side, c->ev_fork, c->ev_join));
    return CSTARK_OK;
}

// ---- K2 / K3 ---------------------------------------------------------------------------------------
uint64_t cstark_field_generator(void) { return cs::host::generator(); }
uint64_t cstark_field_lde_offset(void) { return cs::host::lde_offset(); }
uint64_t cstark_field_root_of_unity(uint32_t log_n) { return log_n <= 55 ? cs::host::root_of_unity(log_n) : 0; }

int cstark_interpolate_columns(cstark_ctx *c, uint64_t *d_evals, uint64_t *d_coeffs, uint32_t width, uint32_t log_n) {
    return interpolate_impl(c, d_evals, d_coeffs, width, log_n);
}
int cstark_lde_columns(cstark_ctx *c, const uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t log_n, uint32_t log_blowup,
                       uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    return lde_impl(c, d_coeffs, d_lde, width, 0, width, log_n, log_blowup, domain_offset, k0, nk);
}
int cstark_step_columns(cstark_ctx *c, uint64_t *d_evals, uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols,
                        uint32_t log_n, uint32_t block_len, uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    return step_impl(c, d_evals, d_coeffs, d_lde, width, col0, ncols, log_n, block_len, 0, log_blowup, domain_offset, k0, nk);
}
int cstark_step2_columns(cstark_ctx *c, uint64_t *d_evals, uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols,
                         uint32_t log_n, uint32_t block_len, uint32_t split, uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    if (split == 0) return fail(CSTARK_ERR_INVALID_ARG, "the split row must lie inside the block");
    return step_impl(c, d_evals, d_coeffs, d_lde, width, col0, ncols, log_n, block_len, split, log_blowup, domain_offset, k0, nk);
}

// ---- composition polynomial (first "next" row: engine into_poly + column split) -----------------------------------
int cstark_composition_columns(cstark_ctx *c, const uint64_t *d_combined, uint64_t *d_cols, uint32_t log_n, uint32_t log_blowup) {
    if (!c || !d_combined || !d_cols) return fail(CSTARK_ERR_INVALID_ARG, "cstark_composition_columns: null argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n + log_blowup > cs::NTT_MAX_LOG_N || log_blowup == 0 || log_blowup > 6)
        return fail(CSTARK_ERR_UNSUPPORTED, "composition domain must be 2^7 .. 2^24 points");
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)1 << (log_n + log_blowup);
    RC_TRY(ensure_ws(c, 2 * N * 8));
    uint64_t *nat = (uint64_t *)c->ws, *h = nat + N;
    if (log_blowup <= 3) {
        // The evaluation domain is the union of b cosets of the n-point domain and the table is coset-major: b interpolations of
        // size n (the register-tiled kernels, cosets as columns), then per row a twist and a b-point inverse DFT across the cosets
        // -- instead of a transposition and one transform of size b n.  Same coefficients (exact arithmetic).
        const NttPlan *pn, *pN;
        RC_TRY(get_plan(c, log_n, &pn));
        RC_TRY(get_plan(c, log_n + log_blowup, &pN));
        cs::NttArgs a{};
        a.in = d_combined; a.scratch = h; a.out = nat; a.width = 1u << log_blowup; a.batch = 1; a.log_n = log_n;
        a.w = pn->winv; a.post_scale = pn->n_inv; a.do_scale = true; a.inverse = true; a.aux = pn->aux_winv;
        HIP_TRY(cs::ntt_columns(a, c->stream));
        const uint64_t b_inv = cs::host::inv(cs::host::from_u64(1ull << log_blowup));
        HIP_TRY(cs::coset_combine(nat, h, log_n, log_blowup, pN->winv, b_inv, c->stream));
        HIP_TRY(cs::split_columns(h, d_cols, log_n, log_blowup, cs::host::inv(cs::host::lde_offset()), c->stream));
        return CSTARK_OK;
    }
    HIP_TRY(cs::interleave_cosets(d_combined, nat, log_n, log_blowup, c->stream));
    // interpolate over the whole evaluation domain (offset handled by the g^-m scaling of the split)
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n + log_blowup, &p));
    cs::NttArgs a{};
    a.in = nat; a.scratch = nat; a.out = h; a.width = 1; a.batch = 1; a.log_n = log_n + log_blowup;
    a.w = p->winv; a.post_scale = p->n_inv; a.do_scale = true; a.inverse = true; a.aux = p->aux_winv;
    HIP_TRY(cs::ntt_columns(a, c->stream));
    HIP_TRY(cs::split_columns(h, d_cols, log_n, log_blowup, cs::host::inv(cs::host::lde_offset()), c->stream));
    return CSTARK_OK;
}

// ---- out-of-domain frame and DEEP composition ("next" rows) -----------------------------------------------------------
int cstark_evaluate_polys_at(cstark_ctx *c, const uint64_t *d_coeffs, uint32_t width, uint32_t log_n, const uint64_t *points, uint32_t npts,
                             uint64_t *out /* host [npts][width] */) {
    if (!c || !d_coeffs || !points || !out || width == 0 || npts == 0 || npts > 16) return fail(CSTARK_ERR_INVALID_ARG, "cstark_evaluate_polys_at: bad argument");
    if (log_n > 30) return fail(CSTARK_ERR_INVALID_ARG, "bad polynomial size");
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = ((size_t)npts + (size_t)npts * width + cs::poly_eval_scratch_words(width, log_n, npts)) * 8;
    if (need > c->desc_bytes) {
        if (c->desc_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->desc_buf)); c->desc_buf = nullptr; c->desc_bytes = 0; }
        HIP_TRY(hipMalloc(&c->desc_buf, need));
        c->desc_bytes = need;
    }
    uint64_t *d_pts = (uint64_t *)c->desc_buf, *d_out = d_pts + npts, *d_scr = d_out + (size_t)npts * width;
    HIP_TRY(hipMemcpyAsync(d_pts, points, (size_t)npts * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::poly_eval(d_coeffs, width, log_n, d_pts, npts, d_out, d_scr, c->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)npts * width * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream));
    return CSTARK_OK;
}

int cstark_deep_composition(cstark_ctx *c, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, uint32_t width, uint32_t n_comp,
                            uint64_t z, const uint64_t *ood_trace, const uint64_t *ood_comp, const uint64_t *alpha, const uint64_t *beta,
                            const uint64_t *delta, uint64_t deg_a, uint64_t deg_b, uint64_t *d_out, uint32_t log_n, uint32_t log_blowup,
                            uint32_t k0, uint32_t nk) {
    if (!c || !d_trace_lde || !d_comp_lde || !ood_trace || !ood_comp || !alpha || !beta || !delta || !d_out || nk == 0 || width == 0 || n_comp == 0)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_deep_composition: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6 || (uint64_t)k0 + nk > (1ull << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *plan;
    RC_TRY(get_plan(c, log_n, &plan));
    const size_t b = (size_t)1 << log_blowup, nco = 2 * (size_t)width + n_comp, words = 2 * nco + b;
    // coefficients | frame | coset offsets through a pinned staging block into a device block of the context: no wait between the upload
    // and the launch (round 3 uploaded from a transient vector and waited)
    if (c->deep_words < words) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->deep_buf) { HIP_TRY(hipFree(c->deep_buf)); c->deep_buf = nullptr; }
        if (c->deep_stage) { HIP_TRY(hipHostFree(c->deep_stage)); c->deep_stage = nullptr; }
        c->deep_words = 0;
        HIP_TRY(hipMalloc((void **)&c->deep_buf, words * 8));
        HIP_TRY(hipHostMalloc((void **)&c->deep_stage, words * 8, hipHostMallocDefault));
        if (!c->deep_ev) HIP_TRY(hipEventCreateWithFlags(&c->deep_ev, hipEventDisableTiming));
        c->deep_words = words;
    } else {
        HIP_TRY(hipEventSynchronize(c->deep_ev));
    }
    uint64_t *blk = c->deep_stage;
    memcpy(blk, alpha, width * 8); memcpy(blk + width, beta, width * 8); memcpy(blk + 2 * width, delta, n_comp * 8);
    memcpy(blk + nco, ood_trace, 2 * (size_t)width * 8); memcpy(blk + nco + 2 * width, ood_comp, n_comp * 8);
    const uint64_t wbn = cs::host::root_of_unity(log_n + log_blowup);
    uint64_t shift = cs::host::lde_offset();
    for (size_t k = 0; k < b; k++) { blk[2 * nco + k] = shift; shift = cs::host::mul(shift, wbn); }
    HIP_TRY(hipMemcpyAsync(c->deep_buf, blk, words * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->deep_ev, c->stream));
    const uint64_t *d = c->deep_buf;
    cs::DeepParams p{};
    p.trace_lde = d_trace_lde; p.comp_lde = d_comp_lde; p.w = plan->w; p.coef = d; p.ood = d + nco; p.shifts = d + 2 * nco; p.out = d_out;
    p.z = z; p.zw = cs::host::mul(z, cs::host::root_of_unity(log_n)); p.zb = cs::host::pow(z, n_comp);
    p.deg_a = deg_a; p.deg_b = deg_b; p.width = width; p.nb = n_comp; p.log_n = log_n; p.k0 = k0;
    HIP_TRY(cs::deep_composition(p, nk, c->stream));
    return CSTARK_OK;
}

// ---- FRI: natural-order view of coset-major evaluations and one folding step ("next" rows) ---------------------------
int cstark_interleave_cosets(cstark_ctx *c, const uint64_t *d_coset_major, uint64_t *d_natural, uint32_t log_n, uint32_t log_blowup) {
    if (!c || !d_coset_major || !d_natural || d_coset_major == d_natural) return fail(CSTARK_ERR_INVALID_ARG, "cstark_interleave_cosets: bad argument");
    if (log_n + log_blowup > 30 || log_blowup > 6) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::interleave_cosets(d_coset_major, d_natural, log_n, log_blowup, c->stream));
    return CSTARK_OK;
}
int cstark_fri_fold4(cstark_ctx *c, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint64_t domain_offset, uint64_t alpha) {
    if (!c || !d_evals || !d_out || d_evals == d_out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_fri_fold4: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "layer size must be 2^6 .. 2^24");
    if (domain_offset == 0 || domain_offset >= cs::host::P || alpha >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "offset / alpha must be field elements");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    HIP_TRY(cs::fri_fold4(d_evals, d_out, log_n, p->winv, cs::host::inv(domain_offset), alpha, cs::host::inv(cs::host::from_u64(4)), c->stream));
    return CSTARK_OK;
}
// folding_factor = 4, 8 or 16 (FriOptions, examples/state-transition.rs:46-47)
int cstark_fri_fold(cstark_ctx *c, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint32_t folding_factor, uint64_t domain_offset, uint64_t alpha) {
    if (!c || !d_evals || !d_out || d_evals == d_out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_fri_fold: bad argument");
    if (folding_factor != 4 && folding_factor != 8 && folding_factor != 16) return fail(CSTARK_ERR_UNSUPPORTED, "FRI folding factor must be 4, 8 or 16");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "layer size must be 2^6 .. 2^24");
    if (domain_offset == 0 || domain_offset >= cs::host::P || alpha >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "offset / alpha must be field elements");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    const unsigned log_f = folding_factor == 4 ? 2 : folding_factor == 8 ? 3 : 4;
    HIP_TRY(cs::fri_fold(d_evals, d_out, log_n, log_f, p->winv, cs::host::inv(domain_offset), alpha, cs::host::inv(cs::host::from_u64(folding_factor)), c->stream));
    return CSTARK_OK;
}

// ---- FieldExtension::Quadratic / Cubic: the same three stages over the degree-m extension (ext.hip) ---------------------------
int cstark_evaluate_polys_at_ext(cstark_ctx *c, const uint64_t *d_coeffs, uint32_t width, uint32_t log_n, uint32_t m, const uint64_t *z, uint64_t *out) {
    if (!c || !d_coeffs || !z || !out || width == 0 || (m != 2 && m != 3)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_evaluate_polys_at_ext: bad argument");
    if (log_n > 30) return fail(CSTARK_ERR_INVALID_ARG, "bad polynomial size");
    for (uint32_t i = 0; i < m; i++) if (z[i] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "the point is not an extension element");
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = ((size_t)m * width + cs::poly_eval_ext_scratch_words(width, log_n, m)) * 8;
    if (need > c->desc_bytes) {
        if (c->desc_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->desc_buf)); c->desc_buf = nullptr; c->desc_bytes = 0; }
        HIP_TRY(hipMalloc(&c->desc_buf, need));
        c->desc_bytes = need;
    }
    uint64_t *d_out = (uint64_t *)c->desc_buf, *d_scr = d_out + (size_t)m * width;
    HIP_TRY(cs::poly_eval_ext(d_coeffs, width, log_n, z, m, d_out, d_scr, c->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)m * width * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream));
    return CSTARK_OK;
}
} // extern "C"

// internal (ctx.h): one FRI layer's coin on the device (Blake3 coin: reseed with the layer root at d_root, draw the folding point: m words
// at d_alpha) and the fold with that point; d_evals: [m][2^log_n] component-major
int fri_coin_fold_dev(cstark_ctx *c, uint32_t *d_seed, const uint8_t *d_root, uint64_t *d_alpha, uint32_t *d_root_out, const uint64_t *d_evals,
                      uint64_t *d_out, uint32_t log_n, uint32_t log_f, uint64_t domain_offset, uint32_t m) {
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "layer size must be 2^6 .. 2^24");
    if (m < 1 || m > 3) return fail(CSTARK_ERR_INVALID_ARG, "fri_coin_fold_dev: bad extension degree");
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    const uint64_t offset_inv = cs::host::inv(domain_offset), inv_f = cs::host::inv(cs::host::from_u64(1ull << log_f));
    if (m == 1) {
        HIP_TRY(cs::fri_coin(d_seed, d_root, d_alpha, d_root_out, c->stream));
        HIP_TRY(cs::fri_fold(d_evals, d_out, log_n, log_f, p->winv, offset_inv, 0, inv_f, c->stream, d_alpha));
    } else {
        HIP_TRY(cs::fri_coin_ext(d_seed, d_root, d_alpha, d_root_out, m, c->stream));
        HIP_TRY(cs::fri_fold_ext(d_evals, d_out, log_n, log_f, p->winv, offset_inv, nullptr, m, inv_f, c->stream, d_alpha));
    }
    return CSTARK_OK;
}
// internal (ctx.h): row hashes of a whole table whose cosets are in block order (blake3.h, lde_coset_slot): leaf b j + k = row j of LDE coset k
int hash_rows_slots(cstark_ctx *c, uint32_t hash_fn, const uint64_t *d_lde, uint8_t *d_leaves, uint32_t width, uint32_t log_n, uint32_t log_blowup, uint32_t log_s) {
    if (!c || !d_lde || !d_leaves || width == 0 || width > 128 || hash_fn > 1 || log_blowup > 6 || log_s > log_blowup || ((uintptr_t)d_leaves & 15) != 0)
        return fail(CSTARK_ERR_INVALID_ARG, "hash_rows_slots: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    if (hash_fn == 1) HIP_TRY(cs::hash_rows_sha3(d_lde, d_leaves, width, log_n, log_blowup, 0, 1u << log_blowup, c->stream, log_s));
    else HIP_TRY(cs::hash_rows(d_lde, d_leaves, width, log_n, log_blowup, 0, 1u << log_blowup, c->stream, log_s));
    return CSTARK_OK;
}
// internal (ctx.h): both halves of the out-of-domain frame with ONE upload, one readback and one wait -- the trace polynomials at
// (z, z w) and the composition columns at z^b; out_trace [2][width], out_comp [n_comp] (host)
int evaluate_ood_frames(cstark_ctx *c, const uint64_t *d_coeffs, uint32_t width, const uint64_t *d_ccoef, uint32_t n_comp, uint32_t log_n,
                        const uint64_t zpts[2], uint64_t zb, uint64_t *out_trace, uint64_t *out_comp) {
    if (!c || !d_coeffs || !d_ccoef || !out_trace || !out_comp || width == 0 || n_comp == 0) return fail(CSTARK_ERR_INVALID_ARG, "evaluate_ood_frames: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n_out = 2 * (size_t)width + n_comp;
    const size_t scr_t = cs::poly_eval_scratch_words(width, log_n, 2), scr_c = cs::poly_eval_scratch_words(n_comp, log_n, 1);
    const size_t need = (4 + n_out + scr_t + scr_c) * 8;
    if (need > c->desc_bytes) {
        if (c->desc_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->desc_buf)); c->desc_buf = nullptr; c->desc_bytes = 0; }
        HIP_TRY(hipMalloc(&c->desc_buf, need));
        c->desc_bytes = need;
    }
    uint64_t *d_pts = (uint64_t *)c->desc_buf, *d_out = d_pts + 4, *d_scr = d_out + n_out;
    const uint64_t pts[3] = {zpts[0], zpts[1], zb};
    HIP_TRY(hipMemcpyAsync(d_pts, pts, sizeof pts, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::poly_eval(d_coeffs, width, log_n, d_pts, 2, d_out, d_scr, c->stream));
    HIP_TRY(cs::poly_eval(d_ccoef, n_comp, log_n, d_pts + 2, 1, d_out + 2 * (size_t)width, d_scr + scr_t, c->stream));
    std::vector<uint64_t> host(n_out); // (pageable on purpose: a pinned landing area measured 0.03 ms SLOWER per proof over these small copies)
    HIP_TRY(hipMemcpyAsync(host.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream));
    memcpy(out_trace, host.data(), 2 * (size_t)width * 8);
    memcpy(out_comp, host.data() + 2 * (size_t)width, (size_t)n_comp * 8);
    return CSTARK_OK;
}

// internal (ctx.h): the same frame with the points and the values staying on the device (the device-side channel): d_pts = z, z w, z^b;
// d_out = T(z)[width] | T(z w)[width] | H_i(z^b)[n_comp]
int ood_frames_dev(cstark_ctx *c, const uint64_t *d_coeffs, uint32_t width, const uint64_t *d_ccoef, uint32_t n_comp, uint32_t log_n, const uint64_t *d_pts,
                   uint64_t *d_out) {
    if (!c || !d_coeffs || !d_ccoef || !d_pts || !d_out || width == 0 || n_comp == 0) return fail(CSTARK_ERR_INVALID_ARG, "ood_frames_dev: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t scr_t = cs::poly_eval_scratch_words(width, log_n, 2), scr_c = cs::poly_eval_scratch_words(n_comp, log_n, 1);
    const size_t need = (scr_t + scr_c) * 8;
    if (need > c->desc_bytes) {
        if (c->desc_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->desc_buf)); c->desc_buf = nullptr; c->desc_bytes = 0; }
        HIP_TRY(hipMalloc(&c->desc_buf, need));
        c->desc_bytes = need;
    }
    uint64_t *d_scr = (uint64_t *)c->desc_buf;
    HIP_TRY(cs::poly_eval(d_coeffs, width, log_n, d_pts, 2, d_out, d_scr, c->stream));
    HIP_TRY(cs::poly_eval(d_ccoef, n_comp, log_n, d_pts + 2, 1, d_out + 2 * (size_t)width, d_scr + scr_t, c->stream));
    return CSTARK_OK;
}
// internal (ctx.h): the context's device scratch block (c->desc_buf) with room for `bytes`.  A prover that must not allocate between
// its launches reserves the largest request of its stages first (ood_frames_dev_scratch_bytes).
int desc_reserve(cstark_ctx *c, size_t bytes) {
    if (bytes <= c->desc_bytes) return CSTARK_OK;
    if (c->desc_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->desc_buf)); c->desc_buf = nullptr; c->desc_bytes = 0; }
    HIP_TRY(hipMalloc(&c->desc_buf, bytes));
    c->desc_bytes = bytes;
    return CSTARK_OK;
}
// scratch of ood_frames_dev (m = 1) / ood_frames_dev_ext (m = 2, 3): the segment sums of the three evaluations, and the raw values of
// the m n_comp component columns (m-tuples) for m > 1
static size_t ood_scratch_words(uint32_t width, uint32_t n_comp, uint32_t log_n, uint32_t m, size_t *scr_t, size_t *scr_c) {
    if (m == 1) { *scr_t = cs::poly_eval_scratch_words(width, log_n, 2); *scr_c = cs::poly_eval_scratch_words(n_comp, log_n, 1); return *scr_t + *scr_c; }
    *scr_t = cs::poly_eval_ext_scratch_words(width, log_n, m); *scr_c = cs::poly_eval_ext_scratch_words(m * n_comp, log_n, m);
    return 2 * *scr_t + *scr_c + (size_t)m * m * n_comp;
}
size_t ood_frames_dev_scratch_bytes(uint32_t width, uint32_t n_comp, uint32_t log_n, uint32_t m) {
    size_t scr_t, scr_c;
    return ood_scratch_words(width, n_comp, log_n, m, &scr_t, &scr_c) * 8;
}
// internal (ctx.h): the frame of an extension-field proof with the point and the values staying on the device.  d_pts = z | z w | z^b
// (m-tuples, where channel.hip wrote them); d_out = T(z)[width] | T(z w)[width] | H_i(z^b)[n_comp], m-tuples: what the host channel
// computes with three cstark_evaluate_polys_at_ext calls and a recombination of the composition columns' components on the host.
int ood_frames_dev_ext(cstark_ctx *c, const uint64_t *d_coeffs, uint32_t width, const uint64_t *d_ccoef, uint32_t n_comp, uint32_t log_n, uint32_t m,
                       const uint64_t *d_pts, uint64_t *d_out) {
    if (!c || !d_coeffs || !d_ccoef || !d_pts || !d_out || width == 0 || n_comp == 0 || (m != 2 && m != 3)) return fail(CSTARK_ERR_INVALID_ARG, "ood_frames_dev_ext: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    size_t scr_t, scr_c;
    RC_TRY(desc_reserve(c, ood_scratch_words(width, n_comp, log_n, m, &scr_t, &scr_c) * 8));
    uint64_t *d_scr = (uint64_t *)c->desc_buf, *d_raw = d_scr + 2 * scr_t + scr_c;
    const size_t mw = (size_t)m * width;
    HIP_TRY(cs::poly_eval_ext(d_coeffs, width, log_n, nullptr, m, d_out, d_scr, c->stream, d_pts));
    HIP_TRY(cs::poly_eval_ext(d_coeffs, width, log_n, nullptr, m, d_out + mw, d_scr + scr_t, c->stream, d_pts + m));
    HIP_TRY(cs::poly_eval_ext(d_ccoef, m * n_comp, log_n, nullptr, m, d_raw, d_scr + 2 * scr_t, c->stream, d_pts + 2 * m));
    HIP_TRY(cs::ood_recombine_ext(d_raw, d_out + 2 * mw, n_comp, m, c->stream));
    return CSTARK_OK;
}
// internal (ctx.h): the quotient sums of an extension-field proof on the first nk cosets, d_out = [m][nk][n], from values that never
// left the device: d_coef = alpha[width] | beta[width] | delta[n_comp], d_ood = the frame, d_scal = z | z w | z^b | deg_a | deg_b (5 m of
// its 8 m words; the three constants k1, k2, k3 are computed into the rest here), d_shifts = the coset offsets.  No upload, no wait.
int deep_composition_ext_dev(cstark_ctx *c, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, uint32_t width, uint32_t n_comp, uint32_t m,
                             const uint64_t *d_coef, const uint64_t *d_ood, uint64_t *d_scal, const uint64_t *d_shifts, uint64_t *d_out, uint32_t log_n,
                             uint32_t log_blowup, uint32_t nk) {
    if (!c || !d_trace_lde || !d_comp_lde || !d_coef || !d_ood || !d_scal || !d_shifts || !d_out || width == 0 || n_comp == 0 || (m != 2 && m != 3))
        return fail(CSTARK_ERR_INVALID_ARG, "deep_composition_ext_dev: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6 || nk == 0 || nk > (1u << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *plan;
    RC_TRY(get_plan(c, log_n, &plan));
    HIP_TRY(cs::deep_ext_consts(d_coef, d_ood, d_scal, width, n_comp, m, c->stream));
    cs::DeepExtParams p{};
    p.trace_lde = d_trace_lde; p.comp_lde = d_comp_lde; p.w = plan->w; p.coef = d_coef; p.shifts = d_shifts; p.out = d_out; p.scal = d_scal;
    p.width = width; p.nb = n_comp; p.log_n = log_n; p.log_b = log_blowup; p.m = m;
    p.nk = nk == (1u << log_blowup) ? 0 : nk;
    HIP_TRY(cs::deep_composition_ext(p, c->stream));
    return CSTARK_OK;
}
// internal (ctx.h): the first nk cosets only, d_out = [m][nk][n]
int deep_composition_ext_cosets(cstark_ctx *c, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, uint32_t width, uint32_t n_comp, uint32_t m,
                                const uint64_t *z, const uint64_t *ood_trace, const uint64_t *ood_comp, const uint64_t *alpha, const uint64_t *beta,
                                const uint64_t *delta, const uint64_t *deg_a, const uint64_t *deg_b, uint64_t *d_out, uint32_t log_n, uint32_t log_blowup,
                                uint32_t nk) {
    if (!c || !d_trace_lde || !d_comp_lde || !z || !ood_trace || !ood_comp || !alpha || !beta || !delta || !deg_a || !deg_b || !d_out || width == 0 || n_comp == 0 ||
        (m != 2 && m != 3))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_deep_composition_ext: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    using namespace cs::host;
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *plan;
    RC_TRY(get_plan(c, log_n, &plan));
    const size_t b = (size_t)1 << log_blowup, nco = (size_t)m * (2 * (size_t)width + n_comp);
    std::vector<uint64_t> blk(nco + b);
    memcpy(blk.data(), alpha, (size_t)m * width * 8);
    memcpy(blk.data() + (size_t)m * width, beta, (size_t)m * width * 8);
    memcpy(blk.data() + (size_t)2 * m * width, delta, (size_t)m * n_comp * 8);
    const uint64_t wbn = root_of_unity(log_n + log_blowup);
    uint64_t shift = lde_offset();
    for (size_t k = 0; k < b; k++) { blk[nco + k] = shift; shift = mul(shift, wbn); }
    const size_t bytes = blk.size() * 8;
    if (bytes > c->desc_bytes) {
        if (c->desc_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->desc_buf)); c->desc_buf = nullptr; c->desc_bytes = 0; }
        HIP_TRY(hipMalloc(&c->desc_buf, bytes));
        c->desc_bytes = bytes;
    }
    HIP_TRY(hipMemcpyAsync(c->desc_buf, blk.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::stream_wait(c->stream));
    cs::DeepExtParams p{};
    p.trace_lde = d_trace_lde; p.comp_lde = d_comp_lde; p.w = plan->w; p.coef = (const uint64_t *)c->desc_buf; p.shifts = p.coef + nco; p.out = d_out;
    const EX zz = ex_load(z, m), zw = ex_scale(zz, root_of_unity(log_n)), zb = ex_pow(zz, n_comp, m), da = ex_load(deg_a, m), db = ex_load(deg_b, m);
    EX k1 = ex_zero(), k2 = ex_zero(), k3 = ex_zero();
    for (uint32_t i = 0; i < width; i++) {
        k1 = ex_add(k1, ex_mul(ex_load(alpha + (size_t)m * i, m), ex_load(ood_trace + (size_t)m * i, m), m));
        k2 = ex_add(k2, ex_mul(ex_load(beta + (size_t)m * i, m), ex_load(ood_trace + (size_t)m * (width + i), m), m));
    }
    for (uint32_t i = 0; i < n_comp; i++) k3 = ex_add(k3, ex_mul(ex_load(delta + (size_t)m * i, m), ex_load(ood_comp + (size_t)m * i, m), m));
    for (int q = 0; q < 3; q++) {
        p.z[q] = zz.c[q]; p.zw[q] = zw.c[q]; p.zb[q] = zb.c[q]; p.deg_a[q] = da.c[q]; p.deg_b[q] = db.c[q];
        p.k1[q] = k1.c[q]; p.k2[q] = k2.c[q]; p.k3[q] = k3.c[q];
    }
    p.width = width; p.nb = n_comp; p.log_n = log_n; p.log_b = log_blowup; p.m = m;
    if (nk > b) return fail(CSTARK_ERR_INVALID_ARG, "coset range exceeds the blowup factor");
    p.nk = nk == b ? 0 : nk;
    HIP_TRY(cs::deep_composition_ext(p, c->stream));
    return CSTARK_OK;
}
extern "C" {
int cstark_deep_composition_ext(cstark_ctx *c, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, uint32_t width, uint32_t n_comp, uint32_t m,
                                const uint64_t *z, const uint64_t *ood_trace, const uint64_t *ood_comp, const uint64_t *alpha, const uint64_t *beta,
                                const uint64_t *delta, const uint64_t *deg_a, const uint64_t *deg_b, uint64_t *d_out, uint32_t log_n, uint32_t log_blowup) {
    if (log_blowup > 6) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    return deep_composition_ext_cosets(c, d_trace_lde, d_comp_lde, width, n_comp, m, z, ood_trace, ood_comp, alpha, beta, delta, deg_a, deg_b, d_out, log_n,
                                       log_blowup, 1u << log_blowup);
}
int cstark_fri_fold4_ext(cstark_ctx *c, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint64_t domain_offset, uint32_t m, const uint64_t *alpha) {
    if (!c || !d_evals || !d_out || !alpha || d_evals == d_out || (m != 2 && m != 3)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_fri_fold4_ext: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "layer size must be 2^6 .. 2^24");
    if (domain_offset == 0 || domain_offset >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "offset must be a nonzero field element");
    for (uint32_t i = 0; i < m; i++) if (alpha[i] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "alpha is not an extension element");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    HIP_TRY(cs::fri_fold4_ext(d_evals, d_out, log_n, p->winv, cs::host::inv(domain_offset), alpha, m, cs::host::inv(cs::host::from_u64(4)), c->stream));
    return CSTARK_OK;
}
int cstark_fri_fold_ext(cstark_ctx *c, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint32_t folding_factor, uint64_t domain_offset, uint32_t m,
                        const uint64_t *alpha) {
    if (!c || !d_evals || !d_out || !alpha || d_evals == d_out || (m != 2 && m != 3)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_fri_fold_ext: bad argument");
    if (folding_factor != 4 && folding_factor != 8 && folding_factor != 16) return fail(CSTARK_ERR_UNSUPPORTED, "FRI folding factor must be 4, 8 or 16");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "layer size must be 2^6 .. 2^24");
    if (domain_offset == 0 || domain_offset >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "offset must be a nonzero field element");
    for (uint32_t i = 0; i < m; i++) if (alpha[i] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "alpha is not an extension element");
    HIP_TRY(hipSetDevice(c->device));
    const NttPlan *p;
    RC_TRY(get_plan(c, log_n, &p));
    const unsigned log_f = folding_factor == 4 ? 2 : folding_factor == 8 ? 3 : 4;
    HIP_TRY(cs::fri_fold_ext(d_evals, d_out, log_n, log_f, p->winv, cs::host::inv(domain_offset), alpha, m, cs::host::inv(cs::host::from_u64(folding_factor)), c->stream));
    return CSTARK_OK;
}

// ---- K4 / K5 ---------------------------------------------------------------------------------------
int cstark_hash_rows(cstark_ctx *c, const uint64_t *d_lde, uint8_t *d_leaves, uint32_t width, uint32_t log_n, uint32_t log_blowup,
                     uint32_t k0, uint32_t nk) {
    if (!c || !d_lde || !d_leaves) return fail(CSTARK_ERR_INVALID_ARG, "cstark_hash_rows: null argument");
    if (width == 0 || width > 128) return fail(CSTARK_ERR_UNSUPPORTED, "row width must be 1..128 elements (single Blake3 chunk)");
    if (log_n > 30 || log_blowup > 6 || (uint64_t)k0 + nk > (1ull << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    if (((uintptr_t)d_leaves & 15) != 0) return fail(CSTARK_ERR_INVALID_ARG, "d_leaves must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::hash_rows(d_lde, d_leaves, width, log_n, log_blowup, k0, nk, c->stream));
    return CSTARK_OK;
}

int cstark_hash_rows_fn(cstark_ctx *c, uint32_t hash_fn, const uint64_t *d_lde, uint8_t *d_leaves, uint32_t width, uint32_t log_n, uint32_t log_blowup,
                        uint32_t k0, uint32_t nk) {
    if (hash_fn == 0) return cstark_hash_rows(c, d_lde, d_leaves, width, log_n, log_blowup, k0, nk);
    if (hash_fn != 1) return fail(CSTARK_ERR_UNSUPPORTED, "hash_fn must be 0 (Blake3_256) or 1 (Sha3_256)");
    if (!c || !d_lde || !d_leaves) return fail(CSTARK_ERR_INVALID_ARG, "cstark_hash_rows_fn: null argument");
    if (width == 0 || width > 128) return fail(CSTARK_ERR_UNSUPPORTED, "row width must be 1..128 elements");
    if (log_n > 30 || log_blowup > 6 || (uint64_t)k0 + nk > (1ull << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    if (((uintptr_t)d_leaves & 15) != 0) return fail(CSTARK_ERR_INVALID_ARG, "d_leaves must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::hash_rows_sha3(d_lde, d_leaves, width, log_n, log_blowup, k0, nk, c->stream));
    return CSTARK_OK;
}
int cstark_merkle_build_fn(cstark_ctx *c, uint32_t hash_fn, uint8_t *d_nodes, uint32_t log_leaves) {
    if (hash_fn == 0) return cstark_merkle_build(c, d_nodes, log_leaves);
    if (hash_fn != 1) return fail(CSTARK_ERR_UNSUPPORTED, "hash_fn must be 0 (Blake3_256) or 1 (Sha3_256)");
    if (!c || !d_nodes) return fail(CSTARK_ERR_INVALID_ARG, "cstark_merkle_build_fn: null argument");
    if (log_leaves == 0 || log_leaves > 30) return fail(CSTARK_ERR_INVALID_ARG, "tree must have 2 .. 2^30 leaves");
    if (((uintptr_t)d_nodes & 15) != 0) return fail(CSTARK_ERR_INVALID_ARG, "d_nodes must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::merkle_build_sha3(d_nodes, log_leaves, c->stream));
    return CSTARK_OK;
}

int cstark_merkle_build(cstark_ctx *c, uint8_t *d_nodes, uint32_t log_leaves) {
    if (!c || !d_nodes) return fail(CSTARK_ERR_INVALID_ARG, "cstark_merkle_build: null argument");
    if (log_leaves == 0 || log_leaves > 30) return fail(CSTARK_ERR_INVALID_ARG, "tree must have 2 .. 2^30 leaves");
    if (((uintptr_t)d_nodes & 15) != 0) return fail(CSTARK_ERR_INVALID_ARG, "d_nodes must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::merkle_build(d_nodes, log_leaves, c->stream));
    return CSTARK_OK;
}

// ---- K6 / K7 ---------------------------------------------------------------------------------------
int cstark_tx_evaluate_transitions(cstark_ctx *c, const uint64_t *d_lde, uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n,
                                   uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    cs::CeParams p;
    RC_TRY(ce_params(c, d_lde, d_out, merkle_depth, log_n, log_blowup, k0, nk, &p));
    HIP_TRY(cs::launch_eval_transitions(p, nk, c->stream));
    return CSTARK_OK;
}

} // extern "C"
int lde_column_range(cstark_ctx *c, const uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols, uint32_t log_n,
                     uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    return lde_impl(c, d_coeffs, d_lde, width, col0, ncols, log_n, log_blowup, domain_offset, k0, nk);
}
int step_column_range(cstark_ctx *c, uint64_t *d_evals, uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols, uint32_t log_n,
                      uint32_t block_len, uint32_t split, uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk) {
    return step_impl(c, d_evals, d_coeffs, d_lde, width, col0, ncols, log_n, block_len, split, log_blowup, domain_offset, k0, nk);
}
int tx_build_trace_split(cstark_ctx *c, uint64_t *d_trace) {
    if (!c || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "tx_build_trace_split: null argument");
    if (!c->wit_buf || c->wit.n_tx == 0) return fail(CSTARK_ERR_INVALID_ARG, "no witness uploaded");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_trace_gen_split(c->wit, d_trace, c->stream, c->side, c->side2, c->ev_fork, c->ev_join, c->ev_mid, c->ev_join2));
    return CSTARK_OK;
}
// m coefficient sets over the same frame (the components of an extension-field proof): the constraint values are computed once.
// The m coefficient sets of a proof into the context's device block (coefficients, then the per-proof tables of the Rescue windows):
// the caller's struct may be transient, so it is copied into a pinned staging block and uploaded from there without waiting.
static constexpr size_t TX_COEF_WORDS = (size_t)cs::CE_MAX_SETS * cs::CE_COEF_WORDS;
static int ensure_coef_buf(cstark_ctx *c) {
    static_assert(sizeof(cstark_tx_coeffs) == cs::CE_COEF_WORDS * 8, "coefficient block layout");
    if (!c->coef_buf) HIP_TRY(hipMalloc((void **)&c->coef_buf, (TX_COEF_WORDS + (size_t)cs::CE_MAX_SETS * cs::CE_RTAB_WORDS) * 8));
    return CSTARK_OK;
}
// internal (ctx.h): the context's device block of composition coefficients (cstark_tx_coeffs layout, CE_MAX_SETS sets CE_COEF_WORDS words
// apart): the device-side channel draws them there, tx_evaluate_constraints_sets(coeffs = null) reads them
int tx_coef_device_block(cstark_ctx *c, uint64_t **d_coef) {
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(ensure_coef_buf(c));
    *d_coef = c->coef_buf;
    return CSTARK_OK;
}
static int upload_coeffs(cstark_ctx *c, const cstark_tx_coeffs *coeffs, uint32_t m, cs::CeParams &p) {
    constexpr size_t COEF_WORDS = TX_COEF_WORDS;
    RC_TRY(ensure_coef_buf(c));
    if (!c->coef_stage) { // the event first: the staging block is only published once both exist
        if (!c->coef_ev) HIP_TRY(hipEventCreateWithFlags(&c->coef_ev, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc(&c->coef_stage, (size_t)cs::CE_MAX_SETS * sizeof(cstark_tx_coeffs), hipHostMallocDefault));
    } else {
        HIP_TRY(hipEventSynchronize(c->coef_ev)); // the previous upload has left the staging block (long ago, normally)
    }
    memcpy(c->coef_stage, coeffs, (size_t)m * sizeof(cstark_tx_coeffs));
    HIP_TRY(hipMemcpyAsync(c->coef_buf, c->coef_stage, (size_t)m * sizeof(cstark_tx_coeffs), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->coef_ev, c->stream));
    p.coef = c->coef_buf;
    p.rtab = c->coef_buf + COEF_WORDS;
    p.m = m;
    return CSTARK_OK;
}

// Descriptor of the merged extension (ntt.h: coset_even_to_odd_merged) for TransactionAir's thirteen split polynomials: five families,
// the alpha table and the beta tables lifted by x^adj_g, g = 0, 1, 2 (the unreduced adjustments: quotient and remainder by n both
// enter).  `hi`: the same term x^adj_0 for the high part of the final addition, which lives in z = y / w_8n (cosets k - 1 = 2, 4, 6).
struct SplitMerge { unsigned log_n = 0; cs::CosetMergeDesc desc; cs::CosetMergeTerm hi; };
static const SplitMerge &tx_split_merge(unsigned log_n) {
    static thread_local SplitMerge sm; // host arithmetic only; rebuilt when the trace length changes
    if (sm.log_n == log_n) return sm;
    const uint64_t n = 1ull << log_n, g = cs::host::lde_offset();
    uint64_t adj[3];
    for (int i = 0; i < 3; i++) adj[i] = cs::host::tx_group_adjustment(i, n, 8 * n);
    static const int first[cs::CE_SPLIT_FAMILIES] = {0, cs::CE_SPLIT_FAM0, 7, 9, 11}, count[cs::CE_SPLIT_FAMILIES] = {4, 3, 2, 2, 2};
    sm.desc = cs::CosetMergeDesc{};
    sm.desc.families = cs::CE_SPLIT_FAMILIES;
    sm.desc.tables_per_set = cs::CE_SPLIT_TABLES;
    sm.desc.raw_family = cs::CE_SPLIT_FAMILIES - 1;
    for (int f = 0; f < cs::CE_SPLIT_FAMILIES; f++) {
        sm.desc.terms[f] = count[f];
        for (int t = 0; t < count[f]; t++) sm.desc.term[f][t] = cs::coset_merge_term(first[f] + t, t ? adj[t - 1] : 0, log_n, g);
    }
    sm.hi = cs::coset_merge_term(0, adj[0], log_n, cs::host::mul(g, cs::host::root_of_unity(log_n + 3)), 2);
    sm.log_n = log_n;
    return sm;
}

// ---- host steps of the degree-split constraint stage --------------------------------------------------------------------------------
// Low-degree parts are evaluated on the four even cosets, interpolated over that 4n-point sub-domain, extended to the odd cosets and
// recombined; the final addition reaches degree 5 (n - 1), so its high part is pinned on LDE coset 1 (constraints.hip, k_final_split).
// TransactionAir (merged and unmerged), its sharded form and SchnorrAir are lists of the steps below.
namespace {

struct SplitStage {
    unsigned log_n;
    size_t n;
    const NttPlan *pn, *p4, *p8; // transforms of n, 4n and 8n points
    const CosetTable *t1;        // offset 1, blowup 8: row k holds the powers of w_8n^k
    hipStream_t stream;
};
int split_stage(cstark_ctx *c, unsigned log_n, SplitStage *s) {
    *s = SplitStage{log_n, (size_t)1 << log_n, nullptr, nullptr, nullptr, nullptr, c->stream};
    RC_TRY(get_plan(c, log_n, &s->pn));
    RC_TRY(get_plan(c, log_n + 2, &s->p4));
    RC_TRY(get_plan(c, log_n + 3, &s->p8));
    return get_coset_table(c, log_n, 3, cs::host::from_u64(1), &s->t1);
}

// Inverse n-point transforms with the 1 / n scaling: `batch` blocks of `width` columns, `batch_stride` words apart in all three arrays
int inverse_columns(const SplitStage &s, const uint64_t *in, uint64_t *scratch, uint64_t *out, unsigned width, unsigned batch = 1, size_t batch_stride = 0) {
    cs::NttArgs a{};
    a.in = in; a.scratch = scratch; a.out = out; a.width = width; a.batch = batch; a.log_n = s.log_n;
    a.in_batch_stride = batch_stride; a.scratch_batch_stride = batch_stride; a.out_batch_stride = batch_stride;
    a.w = s.pn->winv; a.post_scale = s.pn->n_inv; a.do_scale = true; a.inverse = true; a.aux = s.pn->aux_winv;
    HIP_TRY(cs::ntt_columns(a, s.stream));
    return CSTARK_OK;
}

// Coefficient vectors -> values on odd cosets, one batch of `width` columns per coset (scratch and out: width n words apart; in:
// in_batch_stride, 0 = every coset from the same coefficients).  The prescale of batch i is row first + 2 i of the offset-1 table:
//   first = 1: LDE cosets 1, 3, 5, 7 from the coefficients in y = x / g (what coset_even_to_odd writes);
//   first = 2: cosets 3, 5, 7 from the coefficients in z = y / w_8n of a polynomial interpolated on LDE coset 1 -- on coset k the
//              prescale is (w_8n^(k-1))^s, k - 1 = 2, 4, 6.
int forward_to_cosets(const SplitStage &s, unsigned first, const uint64_t *in, uint64_t *scratch, uint64_t *out, unsigned width, size_t in_batch_stride) {
    const CosetTable *t1 = s.t1;
    cs::NttArgs f{};
    f.in = in; f.scratch = scratch; f.out = out; f.width = width; f.batch = first == 1 ? 4 : 3; f.log_n = s.log_n;
    f.w = s.pn->w; f.prescale = t1->s + first * s.n; f.prescale_batch_stride = 2 * s.n; f.do_scale = false; f.inverse = false;
    f.aux = s.pn->aux_w; f.aux_ps = t1->aux ? t1->aux + first * t1->aux_words : nullptr; f.aux_ps_batch_stride = 2 * t1->aux_words;
    f.in_batch_stride = in_batch_stride; f.scratch_batch_stride = (size_t)width * s.n; f.out_batch_stride = (size_t)width * s.n;
    HIP_TRY(cs::ntt_columns(f, s.stream));
    return CSTARK_OK;
}

// interpolants of the even cosets [kc0, kc0 + nkc) -> inputs of the odd cosets' transforms, out = [4 odd cosets][tables][n] (the 4n
// coefficients are never written)
int even_to_odd(const SplitStage &s, const uint64_t *in, uint64_t *out, unsigned tables, unsigned kc0 = 0, unsigned nkc = 4) {
    HIP_TRY(cs::coset_even_to_odd(in, out, s.log_n, tables, s.p4->winv, s.p8->w, cs::host::inv(cs::host::from_u64(4)), s.stream, kc0, nkc));
    return CSTARK_OK;
}

// The stage's arrays in the context's workspace.  region = words of an array of tables x 4 columns, hcol = words of the final addition's
// sums as n-point tables.  fin_hi = [4 odd cosets][hcol]; fin_tco, fin_hm: merged layout only.
struct SplitWs { uint64_t *even, *sa, *sb, *sc, *odd, *fin_direct, *fin_hi, *fin_co, *fin_scr, *fin_tco, *fin_hm; };
int split_ws_unmerged(cstark_ctx *c, size_t region, size_t hcol, SplitWs *w) {
    RC_TRY(ensure_ws(c, (5 * region + 9 * hcol) * 8));
    *w = SplitWs{};
    w->even = (uint64_t *)c->ws; w->sa = w->even + region; w->sb = w->sa + region; w->sc = w->sb + region; w->odd = w->sc + region;
    w->fin_direct = w->odd + region; w->fin_hi = w->fin_direct + hcol; w->fin_co = w->fin_hi + 4 * hcol; w->fin_scr = w->fin_co + hcol /* [3] */;
    return CSTARK_OK;
}
// merged (hcol = 2 m n): the odd cosets hold fregion words of family vectors; the transforms' input and scratch fit the interpolation's
// scratch (2 fregion <= region); fin_hi = [4 odd cosets][m][n], fin_hm and fin_scr = [3][m][n]
int split_ws_merged(cstark_ctx *c, size_t region, size_t fregion, size_t hcol, SplitWs *w) {
    RC_TRY(ensure_ws(c, (3 * region + fregion + 8 * hcol) * 8));
    *w = SplitWs{};
    w->even = (uint64_t *)c->ws; w->sa = w->even + region; w->sb = w->sa + region; w->sc = w->sa + fregion; w->odd = w->sb + region;
    w->fin_direct = w->odd + fregion; w->fin_hi = w->fin_direct + hcol; w->fin_co = w->fin_hi + 2 * hcol; w->fin_tco = w->fin_co + hcol;
    w->fin_hm = w->fin_tco + hcol; w->fin_scr = w->fin_hm + 3 * hcol / 2;
    return CSTARK_OK;
}

// High parts of the final addition's `rows` sums, one transform per sum: with w.fin_direct = their direct evaluation on LDE coset 1 (zero on
// a shard rank that does not hold it), H = (T - Q) / 2 there, interpolated and extended to cosets 3, 5, 7: w.fin_hi = [4 odd cosets][rows][n].
// (first, per_set, tables_per_set): where the sums' tables sit in w.odd (constraints.h, launch_final_hi)
int final_hi_unmerged(const SplitStage &s, const SplitWs &w, unsigned rows, unsigned first, unsigned per_set, unsigned tables_per_set) {
    HIP_TRY(cs::launch_final_hi(w.odd, w.fin_direct, w.fin_hi, cs::host::inv(cs::host::from_u64(2)), s.log_n, rows, first, per_set, tables_per_set, s.stream));
    RC_TRY(inverse_columns(s, w.fin_hi, w.fin_scr, w.fin_co, rows));
    return forward_to_cosets(s, 2, w.fin_co, w.fin_scr, w.fin_hi + (size_t)rows * s.n, rows, 0);
}

// TransactionAir's parts on the even cosets into even = [CE_SPLIT_TABLES m][4][n]: those whose merged polynomials have degree < 4n
// (constraints.hip: the Rescue windows with their flags; the doublings and the additions with the flag factored out), the final addition's
// two sums (they join the tables; their high part follows after the extension) and the three linear groups in one pass over the
// frame (k_lin_all).  pev: part timing; the one pass is reported as lin_a, lin_b = 0.
int tx_even_cosets(const cs::CeParams &p, uint64_t *even, size_t n, hipStream_t stream, hipEvent_t *pev) {
    if (pev) HIP_TRY(hipEventRecord(pev[0], stream));
    HIP_TRY(cs::launch_rounds_setup(p, stream));
    HIP_TRY(cs::launch_rounds_split(p, even, stream));
    if (pev) HIP_TRY(hipEventRecord(pev[1], stream));
    uint64_t *fam_dbl = even + (size_t)cs::CE_SPLIT_FAM0 * 4 * n, *fam_add = fam_dbl + 12 * n, *fam_addbit = fam_add + 8 * n; // 3 | 2 | 2 tables
    HIP_TRY(cs::launch_ec_split(p, 1, fam_dbl, fam_add, stream)); // the doubling of s*G and the addition of G to the same point
    if (pev) HIP_TRY(hipEventRecord(pev[2], stream));
    if (pev) HIP_TRY(hipEventRecord(pev[3], stream)); // (add0: inside the launch before; the event positions stay)
    HIP_TRY(cs::launch_ec_split(p, 3, fam_dbl, nullptr, stream));
    if (pev) HIP_TRY(hipEventRecord(pev[4], stream));
    HIP_TRY(cs::launch_ec_split(p, 4, fam_addbit, fam_add, stream));
    if (pev) HIP_TRY(hipEventRecord(pev[5], stream));
    uint64_t *fam_final = fam_addbit + 8 * n;
    HIP_TRY(cs::launch_final_split(p, -1, fam_final, stream));
    if (pev) HIP_TRY(hipEventRecord(pev[6], stream));
    HIP_TRY(cs::launch_lin_all(p, even, stream));
    if (pev) { HIP_TRY(hipEventRecord(pev[7], stream)); HIP_TRY(hipEventRecord(pev[8], stream)); }
    return CSTARK_OK;
}

} // namespace

// (internal: declared in ctx.h for the prover)
int tx_evaluate_constraints_sets(cstark_ctx *c, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, uint32_t m, const uint64_t pub_inputs[4],
                                 uint64_t *const *d_outs, uint32_t merkle_depth, uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk,
                                 bool input_is_lde, const uint64_t *d_pub) {
    // coeffs == null: the m coefficient sets are already in the context's device block (tx_coef_device_block: set q at CE_COEF_WORDS q);
    // d_pub != null: the 14 public inputs on the device instead of pub_inputs (both: the device-side channel of prove.hip)
    if ((!pub_inputs && !d_pub) || !d_outs) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_evaluate_constraints: null argument");
    if (m < 1 || m > (uint32_t)cs::CE_MAX_SETS) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_evaluate_constraints: 1..3 coefficient sets");
    for (uint32_t q = 1; q < m; q++)
        if (!d_outs[q]) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_evaluate_constraints: null output");
    cs::CeParams p;
    RC_TRY(ce_params(c, d_lde, d_outs[0], merkle_depth, log_n, log_blowup, k0, nk, &p));
    if (coeffs) RC_TRY(upload_coeffs(c, coeffs, m, p));
    else { RC_TRY(ensure_coef_buf(c)); p.coef = c->coef_buf; p.rtab = c->coef_buf + TX_COEF_WORDS; p.m = m; }
    for (uint32_t q = 1; q < m; q++) p.out_ext[q - 1] = d_outs[q];
    for (int i = 0; i < 4; i++) p.pub[i] = pub_inputs ? pub_inputs[i] : 0;
    p.pubd = d_pub;
    static const bool split_env = [] { const char *e = getenv("CSTARK_ROUNDS_SPLIT"); return !e || atoi(e) != 0; }(); // tuning / debugging
    hipEvent_t *pev = c->part_timing ? c->part_ev : nullptr;
    // input_is_lde: d_lde is the extension of columns of degree < n (the prover's own table), which the split evaluation relies on;
    // the public stage entry points evaluate every point directly and are exact for ANY table
    if (split_env && input_is_lde && k0 == 0 && nk == 8 && log_n + 3 <= cs::NTT_MAX_LOG_N) { // (twiddle tables of size 8n)
        // (Part timing: the extension and the recombination are counted with the last part, lin_c.)
        SplitStage st;
        RC_TRY(split_stage(c, log_n, &st));
        const size_t n = st.n;
        const unsigned T = cs::CE_SPLIT_TABLES * m; // every coefficient set has its own block of polynomials
        const size_t region = (size_t)T * 4 * n; // words per array of T x 4 columns
        const size_t hcol = (size_t)2 * m * n;   // the final addition's two sums per set: one n-point table each
        // CSTARK_SPLIT_MERGE=0 (tuning / debugging): every polynomial through its own transforms to the odd cosets
        static const bool split_merge_env = [] { const char *e = getenv("CSTARK_SPLIT_MERGE"); return !e || atoi(e) != 0; }();
        const unsigned F = cs::CE_SPLIT_FAMILIES * m;
        SplitWs w;
        if (split_merge_env) RC_TRY(split_ws_merged(c, region, (size_t)F * 4 * n, hcol, &w));
        else RC_TRY(split_ws_unmerged(c, region, hcol, &w));
        RC_TRY(tx_even_cosets(p, w.even, n, c->stream, pev));
        RC_TRY(inverse_columns(st, w.even, w.sa, w.sb, 4 * T)); // every polynomial on every even coset
        if (split_merge_env) {
            // The recombination inside a flag family is a sum of monomial multiples, i.e. of rotated coefficient vectors: merged where the
            // coefficients sit in registers, five vectors per odd coset and set go through the forward transforms instead of thirteen.
            const SplitMerge &sm = tx_split_merge(log_n);
            HIP_TRY(cs::coset_even_to_odd_merged(w.sb, w.sa, log_n, m, sm.desc, st.p4->winv, st.p8->w, cs::host::inv(cs::host::from_u64(4)), w.fin_tco, c->stream));
            RC_TRY(forward_to_cosets(st, 1, w.sa, w.sc, w.odd, F, (size_t)F * n)); // sa = [4 odd cosets][m][5][n]
            // high part of the final addition, H' = h0 + x^adj_0 h1: on LDE coset 1 from the merged table and the merged direct sums;
            // h0, h1 apart only as coefficients (interpolant of T over coset 1 from the extension kernel, minus that of the direct
            // sums), merged there, then ONE transform per set to each of the cosets 3, 5, 7
            const uint64_t half = cs::host::inv(cs::host::from_u64(2));
            HIP_TRY(cs::launch_final_split(p, 1, w.fin_direct, c->stream));
            HIP_TRY(cs::launch_final_hi_merged(p, w.odd, w.fin_direct, w.fin_hi, half, c->stream));
            RC_TRY(inverse_columns(st, w.fin_direct, w.fin_scr, w.fin_co, 2 * m));
            HIP_TRY(cs::launch_final_hi_merge(p, w.fin_tco, w.fin_co, w.fin_hm, sm.hi, half, c->stream));
            RC_TRY(forward_to_cosets(st, 2, w.fin_hm, w.fin_scr, w.fin_hi + (size_t)m * n, m, (size_t)m * n));
        } else {
            RC_TRY(even_to_odd(st, w.sb, w.sa, T)); // sa = [4 odd cosets][T][n]
            RC_TRY(forward_to_cosets(st, 1, w.sa, w.sc, w.odd, T, (size_t)T * n));
            HIP_TRY(cs::launch_final_split(p, 1, w.fin_direct, c->stream));
            RC_TRY(final_hi_unmerged(st, w, 2 * m, cs::CE_SPLIT_FINAL, 2, cs::CE_SPLIT_TABLES));
        }
        HIP_TRY(cs::launch_split_finish(p, w.even, w.odd, w.fin_hi, c->stream, split_merge_env));
        if (pev) HIP_TRY(hipEventRecord(pev[cs::CE_NUM_PARTS], c->stream));
    } else {
        HIP_TRY(cs::launch_eval_constraints(p, nk, c->stream, pev));
    }
    c->part_valid = c->part_timing;
    return CSTARK_OK;
}
// One rank of a proof sharded by LDE coset: the split evaluation on the rank's even cosets, the extension of its (partial) tables to the
// odd cosets and the recombination of its share (constraints.hip: k_split_finish_shard).  Everything between the even-coset values
// and the merged evaluations of an odd coset is linear in those values, so the ranks' shares add up to what the single-GPU path
// writes; exact field arithmetic, hence bit-identical proofs.
int tx_evaluate_constraints_shard(cstark_ctx *c, const uint64_t *d_lde, const uint64_t *d_coeffs, const cstark_tx_coeffs *coeffs, const uint64_t pub_inputs[4],
                                  uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n, uint32_t k0, uint32_t nk) {
    if (!coeffs || !pub_inputs || !d_out || !d_coeffs) return fail(CSTARK_ERR_INVALID_ARG, "sharded constraint evaluation: null argument");
    if ((nk != 2 && nk != 4) || (k0 % nk) || k0 + nk > 8) return fail(CSTARK_ERR_INVALID_ARG, "sharded split evaluation: a rank holds 2 or 4 consecutive cosets");
    if (log_n + 3 > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_UNSUPPORTED, "trace too long for the split evaluation");
    cs::CeParams p;
    RC_TRY(ce_params(c, d_lde, d_out, merkle_depth, log_n, 3, k0, nk, &p));
    RC_TRY(upload_coeffs(c, coeffs, 1, p));
    for (int i = 0; i < 4; i++) p.pub[i] = pub_inputs[i];
    p.nkc = nk / 2;
    const unsigned kc0 = k0 / 2, nkc = nk / 2;
    SplitStage st;
    RC_TRY(split_stage(c, log_n, &st));
    const size_t n = st.n;
    const unsigned T = cs::CE_SPLIT_TABLES;
    const size_t region = (size_t)T * 4 * n, hcol = (size_t)2 * n;
    // register 37 on all eight cosets first: the extension uses the workspace itself
    uint64_t *bit37 = nullptr;
    {
        if (!c->shard_bit37 || c->shard_bit37_words < 8 * n) {
            if (c->shard_bit37) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->shard_bit37)); c->shard_bit37 = nullptr; }
            HIP_TRY(hipMalloc((void **)&c->shard_bit37, 8 * n * 8));
            c->shard_bit37_words = 8 * n;
        }
        bit37 = c->shard_bit37;
        RC_TRY(lde_impl(c, d_coeffs + (size_t)37 * n, bit37, 1, 0, 1, log_n, 3, cs::host::lde_offset(), 0, 8));
    }
    SplitWs w;
    RC_TRY(split_ws_unmerged(c, region, hcol, &w));
    RC_TRY(tx_even_cosets(p, w.even, n, c->stream, nullptr)); // no part timing
    // interpolation of every table on the rank's even cosets: columns [kc0, kc0 + nkc) of each table's four (batch = table)
    RC_TRY(inverse_columns(st, w.even + (size_t)kc0 * n, w.sa + (size_t)kc0 * n, w.sb + (size_t)kc0 * n, nkc, T, 4 * n));
    RC_TRY(even_to_odd(st, w.sb, w.sa, T, kc0, nkc));
    RC_TRY(forward_to_cosets(st, 1, w.sa, w.sc, w.odd, T, (size_t)T * n));
    // Q, the direct evaluation on LDE coset 1, only on the rank that holds that coset: the ranks' shares of H add up
    if (k0 == 0) HIP_TRY(cs::launch_final_split(p, 1, w.fin_direct, c->stream));
    else HIP_TRY(hipMemsetAsync(w.fin_direct, 0, hcol * 8, c->stream));
    RC_TRY(final_hi_unmerged(st, w, 2, cs::CE_SPLIT_FINAL, 2, cs::CE_SPLIT_TABLES));
    HIP_TRY(cs::launch_split_finish_shard(p, w.even, w.odd, w.fin_hi, bit37, d_out, c->stream));
    return CSTARK_OK;
}
int tx_shard_combine(cstark_ctx *c, const uint64_t *d_parts, uint64_t *d_out, uint32_t log_n, uint32_t nk) {
    if (!c || !d_parts || !d_out || (nk != 2 && nk != 4)) return fail(CSTARK_ERR_INVALID_ARG, "tx_shard_combine: bad argument");
    HIP_TRY(cs::launch_shard_combine(d_parts, d_out, log_n, nk / 2, c->stream));
    return CSTARK_OK;
}

// cstark_schnorr_check_signatures behind its null / count checks.  One device block of the context, grown when needed:
//   messages [count][28] | sig_rx [count][6] | h limbs [count][4] | ladder points [2 count][18] | x [count][6] | sig_s [count][32] | verdicts [count]
// Nothing of the resident witness (c->wit, c->wit_buf, c->tail_buf, the Schnorr statement caches) is read or written.
static_assert(cs::SIG_VALID == CSTARK_SIG_VALID && cs::SIG_MISMATCH == CSTARK_SIG_MISMATCH && cs::SIG_KEY_NOT_ON_CURVE == CSTARK_SIG_KEY_NOT_ON_CURVE &&
                  cs::SIG_SCALAR_RANGE == CSTARK_SIG_SCALAR_RANGE,
              "k_sig_final writes the values of cstark_sig_verdict");
// that block for `count` signatures, carved (also for cstark_tx_witness_check, whose messages and signatures are on the device already)
int signature_block(cstark_ctx *c, uint32_t count, cstark_sig_block *b) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = count, bytes = n * (80 * 8 + 32 + 1);
    if (c->sig_bytes < bytes) {
        if (c->sig_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->sig_buf)); c->sig_buf = nullptr; c->sig_bytes = 0; }
        HIP_TRY(hipMalloc(&c->sig_buf, bytes));
        c->sig_bytes = bytes;
    }
    b->messages = (uint64_t *)c->sig_buf; b->sig_rx = b->messages + 28 * n; b->h_limbs = b->sig_rx + 6 * n; b->points = b->h_limbs + 4 * n;
    b->x = b->points + 36 * n;
    b->sig_s = (uint8_t *)(b->x + 6 * n); b->verdicts = b->sig_s + 32 * n;
    return CSTARK_OK;
}
int signature_check(cstark_ctx *c, const char *who, uint32_t count, const uint64_t *messages, const uint64_t *sig_rx, const uint8_t *sig_s,
                    uint8_t *verdicts, uint64_t *rx_out) {
    char where[96];
    for (size_t i = 0; i < (size_t)28 * count; i++)
        if (messages[i] >= cs::host::P) {
            snprintf(where, sizeof where, "%s: messages[%zu][%zu]", who, i / 28, i % 28);
            return fail(CSTARK_ERR_INVALID_ARG, "%s is not a reduced field element", where);
        }
    for (size_t i = 0; i < (size_t)6 * count; i++)
        if (sig_rx[i] >= cs::host::P) {
            snprintf(where, sizeof where, "%s: sig_rx[%zu][%zu]", who, i / 6, i % 6);
            return fail(CSTARK_ERR_INVALID_ARG, "%s is not a reduced field element", where);
        }
    cstark_sig_block b;
    RC_TRY(signature_block(c, count, &b));
    const size_t n = count;
    uint64_t *d_msg = b.messages, *d_rx = b.sig_rx, *d_h = b.h_limbs, *d_pts = b.points, *d_x = b.x;
    uint8_t *d_s = b.sig_s, *d_verdicts = b.verdicts;
    HIP_TRY(hipMemcpyAsync(d_msg, messages, n * 28 * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_rx, sig_rx, n * 6 * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_s, sig_s, n * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::launch_signature_check(d_msg, d_rx, d_s, d_h, d_pts, d_verdicts, d_x, count, c->stream));
    HIP_TRY(hipMemcpyAsync(verdicts, d_verdicts, n, hipMemcpyDeviceToHost, c->stream));
    if (rx_out) HIP_TRY(hipMemcpyAsync(rx_out, d_x, n * 6 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // synchronous: the verdicts are on the host, the caller's arrays are free again
    return CSTARK_OK;
}

// ---- signing (cstark_schnorr_public_keys, cstark_schnorr_sign_nonces, cstark_schnorr_sign) --------------------------------------------
// They run in the device block of the signature check (c->sig_buf, grown when needed): both kinds of call are synchronous, upload
// everything they read and keep nothing in the block between calls, so sharing it is invisible to either.  The fixed-base table is
// built by the context's first call that signs (sign_table_find, above).  Nothing of the resident witness (c->wit, c->wit_buf,
// c->tail_buf, the Schnorr statement caches) is read or written.
static_assert(cs::SIGN_OK == CSTARK_SIGN_OK && cs::SIGN_NEGATIVE == CSTARK_SIGN_NEGATIVE && cs::SIGN_RANGE == CSTARK_SIGN_RANGE &&
                  cs::SIGN_INFINITY == CSTARK_SIGN_INFINITY && (int)cs::sign::EXHAUSTED == CSTARK_SIGN_EXHAUSTED && (int)cs::sign::OK == CSTARK_SIGN_OK,
              "k_sign_scalar and sign_plan.h write the values of cstark_sign_status");
static_assert(cs::sign::MAX_SECRET == CSTARK_SIG_MAX_SECRET, "the documented cap is the plan's");
namespace {

int sign_scratch(cstark_ctx *c, size_t bytes, const uint64_t **table) {
    HIP_TRY(hipSetDevice(c->device));
    uint64_t *t = sign_table_find(c);
    if (!t) {
        HIP_TRY(hipMalloc(&t, cs::SIGN_TABLE_WORDS * 8));
        const hipError_t e = cs::launch_sign_table(t, c->stream);
        if (e != hipSuccess) { (void)hipFree(t); HIP_TRY(e); }
        sign_table_keep(c, t);
    }
    *table = t;
    if (c->sig_bytes < bytes) {
        if (c->sig_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->sig_buf)); c->sig_buf = nullptr; c->sig_bytes = 0; }
        HIP_TRY(hipMalloc(&c->sig_buf, bytes));
        c->sig_bytes = bytes;
    }
    return CSTARK_OK;
}

// the block of `rows` attempts for n signatures: every array starts on an 8-byte boundary
struct SignBlock {
    uint64_t *msg, *secrets, *gathered, *nonces, *rx, *h, *s;
    uint32_t *owner;
    uint8_t *infinity, *status;
    static size_t bytes(size_t n, size_t rows) { return n * 29 * 8 + rows * (28 + 5 + 6 + 4 + 4) * 8 + (rows * 4 + 7) / 8 * 8 + 2 * rows; }
    SignBlock(void *base, size_t n, size_t rows) {
        msg = (uint64_t *)base; secrets = msg + 28 * n; gathered = secrets + n; nonces = gathered + 28 * rows; rx = nonces + 5 * rows; h = rx + 6 * rows;
        s = h + 4 * rows; owner = (uint32_t *)(s + 4 * rows); infinity = (uint8_t *)owner + (rows * 4 + 7) / 8 * 8; status = infinity + rows;
    }
};

// the misuse rules the three signing calls share; the first offender is named
int sign_arguments(const char *who, uint32_t count, const uint64_t *messages, const uint64_t *secrets, const uint64_t *nonces) {
    char text[160];
    if (count == 0 || count > cs::sign::MAX_COUNT) return fail(CSTARK_ERR_INVALID_ARG, "%s: count must be 1 .. 2^20", who);
    for (uint32_t i = 0; i < count; i++)
        if (secrets[i] == 0 || secrets[i] > cs::sign::MAX_SECRET) {
            snprintf(text, sizeof text, "%s: secrets[%u] is not in 1 .. %u", who, i, (unsigned)cs::sign::MAX_SECRET);
            return fail(CSTARK_ERR_INVALID_ARG, "%s", text);
        }
    if (nonces)
        for (uint32_t i = 0; i < count; i++)
            if (nonces[5 * (size_t)i + 4] >> 8) {
                snprintf(text, sizeof text, "%s: nonces[%u] is not below 2^264", who, i);
                return fail(CSTARK_ERR_INVALID_ARG, "%s", text);
            }
    if (messages)
        for (size_t i = 0; i < (size_t)28 * count; i++)
            if (messages[i] >= cs::host::P) {
                snprintf(text, sizeof text, "%s: messages[%zu][%zu] is not a reduced field element", who, i / 28, i % 28);
                return fail(CSTARK_ERR_INVALID_ARG, "%s", text);
            }
    return CSTARK_OK;
}

} // namespace

int sign_public_keys(cstark_ctx *c, uint32_t count, const uint64_t *secrets, uint64_t *keys_out) {
    const size_t n = count;
    const uint64_t *table;
    RC_TRY(sign_scratch(c, n * (5 + 12) * 8 + n, &table));
    uint64_t *d_nonces = (uint64_t *)c->sig_buf, *d_points = d_nonces + 5 * n;
    uint8_t *d_inf = (uint8_t *)(d_points + 12 * n);
    std::vector<uint64_t> nonces(5 * n, 0); // sk*G by the comb: the nonce is the secret
    for (size_t i = 0; i < n; i++) nonces[5 * i] = secrets[i];
    HIP_TRY(hipMemcpyAsync(d_nonces, nonces.data(), n * 40, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::launch_sign_points(table, d_nonces, d_points, nullptr, d_inf, count, c->stream));
    HIP_TRY(hipMemcpyAsync(keys_out, d_points, n * 96, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CSTARK_OK;
}

static int sign_with_nonces(cstark_ctx *c, uint32_t count, const uint64_t *messages, const uint64_t *secrets, const uint64_t *nonces, uint64_t *sig_rx,
                            uint8_t *sig_s, uint8_t *status) {
    const size_t n = count;
    const uint64_t *table;
    RC_TRY(sign_scratch(c, SignBlock::bytes(n, n), &table));
    const SignBlock b(c->sig_buf, n, n);
    HIP_TRY(hipMemcpyAsync(b.msg, messages, n * 28 * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.secrets, secrets, n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.nonces, nonces, n * 40, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::launch_sign_attempts(table, b.msg, nullptr, nullptr, b.secrets, b.nonces, b.rx, b.infinity, b.h, (uint8_t *)b.s, b.status, count,
                                     c->stream));
    HIP_TRY(hipMemcpyAsync(sig_rx, b.rx, n * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(sig_s, b.s, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, b.status, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CSTARK_OK;
}

int sign_seeded(cstark_ctx *c, uint32_t count, const uint64_t *messages, const uint64_t *secrets, uint64_t seed, uint32_t max_attempts, uint64_t *sig_rx,
                uint8_t *sig_s, uint32_t *attempts_out, uint8_t *status) {
    const size_t n = count;
    cs::sign::Plan plan(count, secrets, seed, max_attempts);
    size_t cap = 0; // rows of the largest round
    for (size_t t = 0; t < n && cap < cs::sign::ROUND_ATTEMPTS; t++) cap += std::min<size_t>((secrets[t] + 2) / 2, max_attempts);
    cap = std::min<size_t>(cap, cs::sign::ROUND_ATTEMPTS);
    const uint64_t *table;
    RC_TRY(sign_scratch(c, SignBlock::bytes(n, cap), &table));
    const SignBlock b(c->sig_buf, n, cap);
    HIP_TRY(hipMemcpyAsync(b.msg, messages, n * 28 * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.secrets, secrets, n * 8, hipMemcpyHostToDevice, c->stream));
    cs::sign::Round round;
    std::vector<uint64_t> rx;
    std::vector<uint8_t> s, st;
    std::vector<std::pair<uint32_t, uint32_t>> accepted;
    while (plan.next_round(round)) {
        const size_t rows = round.rows();
        if (rows > cap) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_schnorr_sign: a round outgrew its scratch");
        rx.resize(6 * rows); s.resize(32 * rows); st.resize(rows);
        HIP_TRY(hipMemcpyAsync(b.owner, round.owner.data(), rows * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(b.nonces, round.nonces.data(), rows * 40, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(cs::launch_sign_attempts(table, b.msg, b.owner, b.gathered, b.secrets, b.nonces, b.rx, b.infinity, b.h, (uint8_t *)b.s, b.status,
                                         (uint32_t)rows, c->stream));
        HIP_TRY(hipMemcpyAsync(st.data(), b.status, rows, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rx.data(), b.rx, rows * 48, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(s.data(), b.s, rows * 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        accepted.clear();
        plan.select(round, st.data(), accepted);
        for (const auto &hit : accepted) {
            memcpy(sig_rx + 6 * (size_t)hit.first, &rx[6 * (size_t)hit.second], 48);
            memcpy(sig_s + 32 * (size_t)hit.first, &s[32 * (size_t)hit.second], 32);
        }
    }
    for (size_t t = 0; t < n; t++) {
        const cs::sign::Signature &sg = plan.sigs[t];
        status[t] = sg.status;
        if (attempts_out) attempts_out[t] = sg.attempts;
        if (sg.status != cs::sign::OK) {
            memset(sig_rx + 6 * t, 0, 48);
            memset(sig_s + 32 * t, 0, 32);
        }
    }
    return CSTARK_OK;
}

extern "C" {

int cstark_schnorr_public_keys(cstark_ctx *c, uint32_t count, const uint64_t *secrets, uint64_t *keys_out) {
    if (!c || !secrets || !keys_out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_public_keys: null argument");
    RC_TRY(sign_arguments("cstark_schnorr_public_keys", count, nullptr, secrets, nullptr));
    return sign_public_keys(c, count, secrets, keys_out);
}

int cstark_schnorr_sign_nonces(cstark_ctx *c, uint32_t count, const uint64_t *messages, const uint64_t *secrets, const uint64_t *nonces, uint64_t *sig_rx,
                               uint8_t *sig_s, uint8_t *status) {
    if (!c || !messages || !secrets || !nonces || !sig_rx || !sig_s || !status) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_sign_nonces: null argument");
    RC_TRY(sign_arguments("cstark_schnorr_sign_nonces", count, messages, secrets, nonces));
    return sign_with_nonces(c, count, messages, secrets, nonces, sig_rx, sig_s, status);
}

int cstark_schnorr_sign(cstark_ctx *c, uint32_t count, const uint64_t *messages, const uint64_t *secrets, uint64_t seed, uint32_t max_attempts,
                        uint64_t *sig_rx, uint8_t *sig_s, uint32_t *attempts_out, uint8_t *status) {
    if (!c || !messages || !secrets || !sig_rx || !sig_s || !status) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_sign: null argument");
    RC_TRY(sign_arguments("cstark_schnorr_sign", count, messages, secrets, nullptr));
    if (max_attempts == 0 || max_attempts > cs::sign::MAX_ATTEMPTS) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_sign: max_attempts must be 1 .. 4096");
    return sign_seeded(c, count, messages, secrets, seed, max_attempts, sig_rx, sig_s, attempts_out, status);
}

} // extern "C"

extern "C" {

int cstark_tx_evaluate_constraints(cstark_ctx *c, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, const uint64_t pub_inputs[4],
                                   uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    uint64_t *outs[1] = {d_out};
    return tx_evaluate_constraints_sets(c, d_lde, coeffs, 1, pub_inputs, outs, merkle_depth, log_n, log_blowup, k0, nk, false);
}

int cstark_tx_evaluate_constraints_lde(cstark_ctx *c, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, const uint64_t pub_inputs[4],
                                       uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n) {
    uint64_t *outs[1] = {d_out};
    return tx_evaluate_constraints_sets(c, d_lde, coeffs, 1, pub_inputs, outs, merkle_depth, log_n, 3, 0, 8, true);
}

int cstark_tx_evaluate_constraints_ext(cstark_ctx *c, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, uint32_t m, const uint64_t pub_inputs[4],
                                       uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    if (!d_out || m < 1 || m > 3) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_evaluate_constraints_ext: bad argument");
    const size_t comp = (size_t)nk << log_n;
    uint64_t *outs[3] = {d_out, d_out + comp, d_out + 2 * comp};
    return tx_evaluate_constraints_sets(c, d_lde, coeffs, m, pub_inputs, outs, merkle_depth, log_n, log_blowup, k0, nk, false);
}

int cstark_tx_evaluate_constraints_ext_lde(cstark_ctx *c, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, uint32_t m,
                                           const uint64_t pub_inputs[4], uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n) {
    if (!d_out || m < 1 || m > 3) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_evaluate_constraints_ext_lde: bad argument");
    const size_t comp = (size_t)8 << log_n;
    uint64_t *outs[3] = {d_out, d_out + comp, d_out + 2 * comp};
    return tx_evaluate_constraints_sets(c, d_lde, coeffs, m, pub_inputs, outs, merkle_depth, log_n, 3, 0, 8, true);
}

// ---- standalone sub-AIRs -------------------------------------------------------------
int cstark_merkle_build_trace(cstark_ctx *c, uint64_t *d_trace) {
    if (!c || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "cstark_merkle_build_trace: null argument");
    if (!c->wit_buf || c->wit.n_tx == 0) return fail(CSTARK_ERR_INVALID_ARG, "no witness uploaded");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_merkle_trace(c->wit, d_trace, c->stream));
    return CSTARK_OK;
}
int cstark_range_build_trace(cstark_ctx *c, uint64_t number, uint64_t *d_trace) {
    if (!c || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "cstark_range_build_trace: null argument");
    if (number >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "number is not a field element");
    const uint64_t canonical = cs::host::to_u64(number);
    if (canonical >> 63) return fail(CSTARK_ERR_INVALID_ARG, "range proofs cover 63-bit values (src/range/tests.rs:54-62 panics above)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_range_trace(canonical, d_trace, c->stream));
    return CSTARK_OK;
}
// Synthetic long form of the range accumulator (BASELINE.json "range-proof AIR, 2^16 steps"; the reference's trace is fixed at 64
// rows): words = the n/64 little-endian words of an (n-1)-bit integer V, host memory.  *number_out (optional) = V mod p, memory form.
int cstark_range_build_trace_bits(cstark_ctx *c, const uint64_t *words, uint32_t log_n, uint64_t *d_trace, uint64_t *number_out) {
    if (!c || !words || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "cstark_range_build_trace_bits: null argument");
    if (log_n < 6 || log_n > 21) return fail(CSTARK_ERR_INVALID_ARG, "trace length must be 2^6 .. 2^21");
    const size_t nw = (size_t)1 << (log_n - 6);
    if (words[nw - 1] >> 63) return fail(CSTARK_ERR_INVALID_ARG, "the value must have at most n - 1 bits (top bit of the last word clear)");
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(ensure_ws(c, 2 * nw * 8));
    uint64_t *d_words = (uint64_t *)c->ws, *d_prefix = d_words + nw;
    HIP_TRY(hipMemcpyAsync(d_words, words, nw * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cs::launch_range_trace_bits(d_words, d_prefix, d_trace, log_n, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the caller's words may be transient
    if (number_out) { // Horner in base 2^64, most significant word first
        uint64_t v = 0;
        const uint64_t B = cs::host::R2; // 2^64 in memory form
        for (size_t i = nw; i-- > 0;) v = cs::host::add(cs::host::mul(v, B), cs::host::from_u64(words[i] % cs::host::P));
        *number_out = v;
    }
    return CSTARK_OK;
}

// SchnorrAir (src/schnorr): messages [n][28], signatures (R.x [n][6], s bytes [n][32]); host arrays are copied
int cstark_schnorr_witness_upload(cstark_ctx *c, uint32_t n_sig, const uint64_t *messages, const uint64_t *sig_rx, const uint8_t *sig_s) {
    if (!c || !messages || !sig_rx || !sig_s || n_sig == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_witness_upload: bad argument");
    // reuse the transaction-witness device view: message[0..12] -> s_old[0..12], [12..24] -> r_old[0..12], [24] -> deltas,
    // [25] -> s_old[13]; the two trailing elements go to msg_tail
    std::vector<uint64_t> s_old((size_t)n_sig * 14, 0), r_old((size_t)n_sig * 14, 0), deltas(n_sig), zeros((size_t)n_sig * 28, 0), tail((size_t)n_sig * 2);
    for (uint32_t t = 0; t < n_sig; t++) {
        const uint64_t *m = messages + 28 * (size_t)t;
        memcpy(&s_old[14 * (size_t)t], m, 12 * 8);
        s_old[14 * (size_t)t + 13] = m[25];
        memcpy(&r_old[14 * (size_t)t], m + 12, 12 * 8);
        deltas[t] = m[24];
        tail[2 * (size_t)t] = m[26];
        tail[2 * (size_t)t + 1] = m[27];
    }
    cstark_tx_witness w{};
    w.n_tx = n_sig; w.merkle_depth = 3;
    w.initial_roots = zeros.data(); w.final_root = zeros.data(); w.s_old_values = s_old.data(); w.r_old_values = r_old.data();
    w.s_indices = zeros.data(); w.r_indices = zeros.data(); w.s_paths = zeros.data(); w.r_paths = zeros.data();
    w.deltas = deltas.data(); w.sig_rx = sig_rx; w.sig_s = sig_s;
    RC_TRY(cstark_tx_witness_upload(c, &w));
    if (c->tail_bytes < tail.size() * 8) {
        if (c->tail_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->tail_buf)); c->tail_buf = nullptr; c->tail_bytes = 0; }
        HIP_TRY(hipMalloc((void **)&c->tail_buf, tail.size() * 8));
        c->tail_bytes = tail.size() * 8;
    }
    HIP_TRY(hipMemcpyAsync(c->tail_buf, tail.data(), tail.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->wit.msg_tail = c->tail_buf;
    c->schnorr_rx.assign(sig_rx, sig_rx + (size_t)n_sig * 6);
    c->schnorr_pub.assign(messages, messages + (size_t)n_sig * 28);
    c->schnorr_pub.insert(c->schnorr_pub.end(), sig_rx, sig_rx + (size_t)n_sig * 6);
    c->schnorr_s.assign(sig_s, sig_s + (size_t)n_sig * 32);
    memset(c->schnorr_seed_key, 0, sizeof c->schnorr_seed_key); // another witness: the cached channel seed is stale
    return CSTARK_OK;
}
int cstark_schnorr_build_trace(cstark_ctx *c, uint64_t *d_trace) {
    if (!c || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_build_trace: null argument");
    if (!c->wit_buf || c->wit.n_tx == 0 || !c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no Schnorr witness uploaded");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_schnorr_trace(c->wit, d_trace, c->stream));
    return CSTARK_OK;
}
int cstark_schnorr_aux_columns(cstark_ctx *c, uint64_t *d_out) {
    if (!c || !d_out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_aux_columns: null argument");
    if (!c->wit_buf || c->wit.n_tx == 0 || !c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no Schnorr witness uploaded");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_schnorr_aux_columns(c->wit, d_out, c->stream));
    return CSTARK_OK;
}
int cstark_schnorr_check_signatures(cstark_ctx *c, uint32_t count, const uint64_t *messages, const uint64_t *sig_rx, const uint8_t *sig_s,
                                    uint8_t *verdicts, uint64_t *rx_out) {
    if (!c || !messages || !sig_rx || !sig_s || !verdicts) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_check_signatures: null argument");
    if (count == 0 || count > (1u << 20)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_check_signatures: count must be 1 .. 2^20");
    return signature_check(c, "cstark_schnorr_check_signatures", count, messages, sig_rx, sig_s, verdicts, rx_out);
}
int cstark_schnorr_mask_columns(uint64_t *out /* [36][512] host */) {
    if (!out) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    std::vector<uint64_t> cols;
    cs::host::schnorr_mask_columns(cols);
    memcpy(out, cols.data(), cols.size() * 8);
    return CSTARK_OK;
}
int cstark_schnorr_evaluate_transitions(cstark_ctx *c, const uint64_t *d_lde, const uint64_t *d_aux_lde, uint64_t *d_out, uint32_t log_n,
                                        uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    if (!c || !d_lde || !d_aux_lde || !d_out || nk == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_evaluate_transitions: bad argument");
    if (log_n < 9 || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6 || (uint64_t)k0 + nk > (1ull << log_blowup)) return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    HIP_TRY(hipSetDevice(c->device));
    const PeriodicTable *pt;
    RC_TRY(get_small_periodic(c, CSTARK_AIR_SCHNORR, 0, log_n, log_blowup, &pt));
    HIP_TRY(cs::launch_eval_transitions_schnorr(d_lde, d_aux_lde, pt->tab, d_out, log_n, k0, nk, c->stream));
    return CSTARK_OK;
}

int cstark_air_shape(int air, uint32_t n_items, uint32_t *width, uint32_t *n_constraints, uint32_t *n_assertions, uint32_t *log_ce_blowup) {
    cs::host::AirShape s;
    if (!cs::host::air_shape(air, s, n_items) || !width || !n_constraints || !n_assertions || !log_ce_blowup) return fail(CSTARK_ERR_UNSUPPORTED, "AIR not available through the generic entry points");
    *width = s.width; *n_constraints = s.n_constraints; *n_assertions = (uint32_t)s.a_reg.size(); *log_ce_blowup = s.log_ce_blowup();
    return CSTARK_OK;
}
int cstark_air_constraint_degree(int air, uint32_t n_items, uint32_t i, uint32_t *base, uint32_t *cycles) {
    cs::host::AirShape s;
    if (!cs::host::air_shape(air, s, n_items) || i >= s.n_constraints || !base || !cycles) return fail(CSTARK_ERR_INVALID_ARG, "bad AIR / constraint index");
    *base = s.base[i]; *cycles = s.cycles[i];
    return CSTARK_OK;
}
int cstark_merkle_periodic_columns(uint32_t merkle_depth, uint64_t *out /* [33][512] host */) {
    std::vector<uint64_t> cols;
    if (!out || !cs::host::merkle_periodic_columns(merkle_depth, cols)) return fail(CSTARK_ERR_INVALID_ARG, "unsupported Merkle depth");
    memcpy(out, cols.data(), cols.size() * 8);
    return CSTARK_OK;
}

int cstark_rescue_chain_periodic_columns(uint64_t *out /* [29][8] host */) {
    if (!out) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    std::vector<uint64_t> cols;
    cs::host::rescue_chain_periodic_columns(cols);
    memcpy(out, cols.data(), cols.size() * 8);
    return CSTARK_OK;
}
// RescueProver::build_trace (benches/rescue.rs:277-322): 14 x 8 * chain_length
int cstark_rescue_chain_build_trace(cstark_ctx *c, const uint64_t seed[7], uint32_t chain_length, uint64_t *d_trace) {
    if (!c || !seed || !d_trace) return fail(CSTARK_ERR_INVALID_ARG, "cstark_rescue_chain_build_trace: null argument");
    if (chain_length < 8 || (chain_length & (chain_length - 1)) || chain_length > (1u << 21)) // benches/rescue.rs:34-37: a power of two
        return fail(CSTARK_ERR_INVALID_ARG, "chain length must be a power of two, 8 .. 2^21 (64 .. 2^24 trace rows)");
    for (int i = 0; i < 7; i++) if (seed[i] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "seed is not a field element");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cs::launch_rescue_chain_trace(seed, chain_length, d_trace, c->stream));
    return CSTARK_OK;
}
int cstark_air_evaluate_transitions(cstark_ctx *c, int air, const uint64_t *d_lde, uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n,
                                    uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    if (!c || !d_lde || !d_out || nk == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_evaluate_transitions: bad argument");
    if (log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6 || (uint64_t)k0 + nk > (1ull << log_blowup))
        return fail(CSTARK_ERR_INVALID_ARG, "bad domain parameters");
    HIP_TRY(hipSetDevice(c->device));
    if (air == CSTARK_AIR_RANGE) {
        HIP_TRY(cs::launch_eval_transitions_range(d_lde, d_out, log_n, nk, c->stream));
        return CSTARK_OK;
    }
    if (air == CSTARK_AIR_RESCUE_CHAIN) {
        const PeriodicTable *pt;
        RC_TRY(get_small_periodic(c, air, 0, log_n, log_blowup, &pt));
        HIP_TRY(cs::launch_eval_transitions_rescue(d_lde, pt->tab, d_out, log_n, k0, nk, c->stream));
        return CSTARK_OK;
    }
    if (air != CSTARK_AIR_MERKLE_UPDATE) return fail(CSTARK_ERR_UNSUPPORTED, "AIR not available through the generic entry points");
    if (log_n < 9) return fail(CSTARK_ERR_INVALID_ARG, "the trace must hold at least one 512-row transaction");
    const PeriodicTable *pt;
    RC_TRY(get_small_periodic(c, air, merkle_depth, log_n, log_blowup, &pt));
    HIP_TRY(cs::launch_eval_transitions_merkle(d_lde, pt->tab, d_out, log_n, k0, nk, c->stream));
    return CSTARK_OK;
}
// coefficient columns [12][n] of the value polynomials of SchnorrAir's sequence assertions (R.x at step 0 and at step 511 of
// every 512-row block, src/schnorr/air.rs:172-224); the caller extends them with cstark_lde_columns
int cstark_schnorr_assertion_polys(cstark_ctx *c, uint64_t *d_out, uint32_t log_n) {
    if (!c || !d_out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_assertion_polys: null argument");
    const size_t n = (size_t)1 << log_n, m = c->schnorr_rx.size() / 6;
    if (m == 0 || m * 512 != n) return fail(CSTARK_ERR_INVALID_ARG, "no Schnorr witness uploaded for this trace length");
    unsigned log_m = 0;
    while (((size_t)1 << log_m) < m) log_m++;
    // Only the first m = n / 512 coefficients of a column are non-zero (the polynomials have degree < m): they are staged in a
    // buffer of the context and copied as 12 rows of m words into the zero-filled columns -- 48 KB at 2^18 rows.  (Round 3 built
    // the 12 n words on the host and uploaded all of them, 25 MB of zeros per proof through the runtime's staging chunks: 0.6 ms of
    // copies on the stream that the interpolation of registers 37..55 waits on, and a host synchronisation.)
    std::vector<uint64_t> &cols = c->schnorr_av_stage;
    cols.assign(12 * m, 0);
    const uint64_t winv = cs::host::inv(cs::host::root_of_unity(log_n));
    for (int half = 0; half < 2; half++) {
        const uint64_t off = cs::host::pow(winv, half ? 511 : 0); // c(x) = P(x * w^-first_step)
        for (int k = 0; k < 6; k++) {
            uint64_t *o = cols.data() + (size_t)(6 * half + k) * m;
            for (size_t t = 0; t < m; t++) o[t] = c->schnorr_rx[6 * t + k];
            if (m > 1) cs::host::intt_small(o, log_m);
            uint64_t sc = cs::host::ONE;
            for (size_t t = 0; t < m; t++) { o[t] = cs::host::mul(o[t], sc); sc = cs::host::mul(sc, off); }
        }
    }
    HIP_TRY(hipMemsetAsync(d_out, 0, 12 * n * 8, c->stream));
    HIP_TRY(hipMemcpy2DAsync(d_out, n * 8, cols.data(), m * 8, m * 8, 12, hipMemcpyHostToDevice, c->stream));
    return CSTARK_OK;
}

} // extern "C"

// ---- host steps of the sub-AIR constraint stage (ctx.h: AirStageRequest) --------------------------------------------------------------
namespace {

static_assert(cs::AIR_MAX_GROUPS == cs::host::AIR_MAX_GROUPS, "air_groups.h groups for the parameter block of constraints.h");
using cs::AirStageRequest;
using cs::AirTransitions;

// the checks of a request, in the order their status codes have always had; fills the AIR's shape
int air_stage_validate(cstark_ctx *c, const AirStageRequest &rq, cs::host::AirShape &s) {
    const bool no_source = (rq.source == AirTransitions::Materialised && !rq.d_evals) || (rq.source == AirTransitions::SchnorrFused && !rq.d_aux_lde);
    if (!c || !rq.d_lde || no_source || (!rq.d_coefs && (!rq.t_alpha || !rq.t_beta || !rq.b_alpha || !rq.b_beta)) || !rq.d_out || rq.nk == 0)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_combine: null argument");
    if (rq.source == AirTransitions::SchnorrFused && (rq.air != CSTARK_AIR_SCHNORR || rq.log_n < 9)) return fail(CSTARK_ERR_INVALID_ARG, "the fused evaluator is SchnorrAir's");
    if (rq.source == AirTransitions::MerkleFused && (rq.air != CSTARK_AIR_MERKLE_UPDATE || rq.log_n < 9)) return fail(CSTARK_ERR_INVALID_ARG, "the fused evaluator is MerkleAir's");
    if (!cs::host::air_shape(rq.air, s, rq.n_items)) return fail(CSTARK_ERR_UNSUPPORTED, "AIR not available through the generic entry points");
    if (s.a_const.empty() && !rq.assertion_values && !rq.d_avalues) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_combine: assertion values required");
    if (rq.d_coefs && s.n_constraints > 115) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_air_combine: device coefficient block holds at most 115 constraints");
    if (rq.log_blowup < s.log_ce_blowup() || rq.log_blowup > 6 || (uint64_t)rq.k0 + rq.nk > (1ull << rq.log_blowup))
        return fail(CSTARK_ERR_INVALID_ARG, "blowup factor below the constraint degree");
    if (rq.log_n < cs::NTT_MIN_LOG_N || rq.log_n > cs::NTT_MAX_LOG_N) return fail(CSTARK_ERR_INVALID_ARG, "bad trace length");
    bool needs_avals = false;
    for (int32_t q : s.a_seq) needs_avals |= q >= 0;
    if (needs_avals && (!rq.d_avals_lde || rq.n_avals == 0)) return fail(CSTARK_ERR_INVALID_ARG, "this AIR has sequence assertions: pass the extended value polynomials");
    if (rq.log_blowup > 3) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_air_combine: blowup factor at most 8");
    return CSTARK_OK;
}

// Everything that depends on (AIR, items, trace length, blowup) only: the degree / divisor groups and the powers of the coset offsets
// (air_groups.h), the assertion tables on the device, the cached divisor inverses -- built once per context and key (rebuilt per call
// it was ~150 modular exponentiations and a blocking upload between the trace root and the evaluation launches of EVERY sub-AIR
// proof).  Nothing enters the context's caches before the whole entry is complete.
int get_air_static(cstark_ctx *c, const AirStageRequest &rq, const cs::host::AirShape &s, const cs::AirCombineStatic **out) {
    const uint32_t log_n = rq.log_n, log_b = rq.log_blowup;
    for (const cs::AirCombineStatic &q : c->air_static)
        if (q.air == rq.air && q.n_items == rq.n_items && q.log_n == log_n && q.log_b == log_b) { *out = &q; return CSTARK_OK; }
    const NttPlan *plan;
    RC_TRY(get_plan(c, log_n, &plan));
    cs::host::AirGroups grp;
    switch (cs::host::air_groups(s, log_n, log_b, grp)) {
    case cs::host::AIR_GROUPS_TOO_MANY_DEGREES: return fail(CSTARK_ERR_UNSUPPORTED, "too many distinct constraint degrees");
    case cs::host::AIR_GROUPS_TOO_MANY_DIVISORS: return fail(CSTARK_ERR_UNSUPPORTED, "too many distinct assertion divisors");
    case cs::host::AIR_GROUPS_OK: break;
    }
    const uint64_t n = 1ull << log_n, b = 1ull << log_b;
    const size_t nc = s.n_constraints, na = s.a_reg.size();
    cs::AirCombineStatic q{};
    q.air = rq.air; q.n_items = rq.n_items; q.log_n = log_n; q.log_b = log_b;
    q.t_grp = grp.t_grp;
    cs::AirCombineParams &p = q.p;
    p.n_tgrp = grp.n_tgrp; p.n_agrp = grp.n_agrp;
    memcpy(p.tgrp_adj, grp.tgrp_adj, sizeof p.tgrp_adj); memcpy(p.agrp_m, grp.agrp_m, sizeof p.agrp_m);
    memcpy(p.agrp_zc, grp.agrp_zc, sizeof p.agrp_zc); memcpy(p.agrp_badj, grp.agrp_badj, sizeof p.agrp_badj);
    memcpy(p.tgrp_shift, grp.tgrp_shift, sizeof p.tgrp_shift); memcpy(p.agrp_bshift, grp.agrp_bshift, sizeof p.agrp_bshift);
    memcpy(p.agrp_mshift, grp.agrp_mshift, sizeof p.agrp_mshift); memcpy(p.zinv_coset, grp.zinv_coset, sizeof p.zinv_coset);
    // device block of the static part: shifts[b] | built-in assertion constants[na] (u64), then u32: a_reg | a_seq | a_grp | t_grp
    std::vector<uint64_t> blk(b + na + (3 * na + nc + 1) / 2 + 1);
    for (uint64_t k = 0; k < b; k++) blk[k] = grp.shifts[k];
    for (size_t a = 0; a < na; a++) blk[b + a] = s.a_const.empty() ? 0 : s.a_const[a];
    uint32_t *q32 = (uint32_t *)(blk.data() + b + na);
    for (size_t a = 0; a < na; a++) q32[a] = s.a_reg[a];
    for (size_t a = 0; a < na; a++) ((int32_t *)q32)[na + a] = s.a_seq.empty() ? -1 : s.a_seq[a];
    for (size_t a = 0; a < na; a++) q32[2 * na + a] = grp.a_grp[a];
    for (size_t i = 0; i < nc; i++) q32[3 * na + i] = grp.t_grp[i];
    DevGuard g;
    HIP_TRY(g.alloc(&q.d_static, blk.size() * 8));
    HIP_TRY(hipMemcpy(q.d_static, blk.data(), blk.size() * 8, hipMemcpyHostToDevice));
    p.shifts = q.d_static;
    p.a_reg = (const uint32_t *)(q.d_static + b + na); p.a_seq = (const int32_t *)(p.a_reg + na);
    p.a_grp = p.a_reg + 2 * na; p.t_grp = p.a_reg + 3 * na;
    p.w = plan->w;
    p.w_last = cs::host::inv(cs::host::root_of_unity(log_n));
    p.width = s.width; p.n_constraints = (uint32_t)nc; p.n_assertions = (uint32_t)na;
    p.stride = 1u << (log_b - s.log_ce_blowup()); p.log_n = log_n;
    // 1 / (x^m - zc) of every assertion divisor over the domain: cached per (m, zc, trace length, blowup).
    // CSTARK_AIR_INV_TABLES=0 (tuning / debugging): one inversion per point inside k_air_combine
    static const bool inv_tables = [] { const char *e = getenv("CSTARK_AIR_INV_TABLES"); return !e || atoi(e) != 0; }();
    std::vector<cs::AssertInverseTable> built; // the divisors no earlier AIR of this context has had
    for (uint32_t gi = 0; inv_tables && gi < p.n_agrp; gi++) {
        for (const cs::AssertInverseTable &t : c->assert_inv)
            if (t.log_n == log_n && t.log_b == log_b && t.m == p.agrp_m[gi] && t.zc == p.agrp_zc[gi]) p.agrp_inv[gi] = t.tab;
        if (p.agrp_inv[gi]) continue;
        cs::AssertInverseTable t{log_n, log_b, p.agrp_m[gi], p.agrp_zc[gi], nullptr};
        HIP_TRY(g.alloc(&t.tab, (size_t)b * (n / t.m) * 8));
        uint64_t sm[8] = {};
        for (uint64_t k = 0; k < b; k++) sm[k] = p.agrp_mshift[k][gi];
        HIP_TRY(cs::launch_assert_inverses(t.tab, plan->w, sm, (unsigned)b, t.m, t.zc, log_n, c->stream));
        p.agrp_inv[gi] = t.tab;
        built.push_back(t);
    }
    g.release();
    for (const cs::AssertInverseTable &t : built) c->assert_inv.push_back(t);
    c->air_static.push_back(std::move(q));
    *out = &c->air_static.back();
    return CSTARK_OK;
}

// The per-proof block of the context: t_alpha | t_beta | b_alpha | b_beta | a_value | the transition coefficients once more in the
// cstark_tx_coeffs layout (SchnorrAir's split evaluation reads alpha[i] at word i, beta[i] at word 115 + i) | device scratch of
// k_merkle_rounds.  Host coefficients go through a pinned staging block, no wait for the caller's arrays; device coefficients
// (rq.d_coefs = alpha[115] | beta[115] | b_alpha[na] | b_beta[na], what channel.hip draws with stride 115) are read where they are,
// the block then serves as the scratch alone.  Sets p's coefficient pointers; *d_txl: the cstark_tx_coeffs layout, *d_rtab: the scratch.
int stage_air_coefs(cstark_ctx *c, const AirStageRequest &rq, const cs::host::AirShape &s, const cs::AirCombineStatic &st, cs::AirCombineParams &p,
                    const uint64_t **d_txl, uint64_t **d_rtab) {
    constexpr size_t TXL = 230;
    const size_t nc = s.n_constraints, na = s.a_reg.size();
    const size_t words = 2 * nc + 3 * na + TXL, total = words + cs::MERKLE_RTAB_WORDS;
    if (c->air_coef_words < total) {
        if (rq.d_coefs && c->air_coef_words) HIP_TRY(hipEventSynchronize(c->air_coef_ev));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->air_coef_buf) { HIP_TRY(hipFree(c->air_coef_buf)); c->air_coef_buf = nullptr; }
        if (c->air_coef_stage) { HIP_TRY(hipHostFree(c->air_coef_stage)); c->air_coef_stage = nullptr; }
        c->air_coef_words = 0;
        HIP_TRY(hipMalloc((void **)&c->air_coef_buf, total * 8));
        HIP_TRY(hipHostMalloc((void **)&c->air_coef_stage, total * 8, hipHostMallocDefault));
        if (!c->air_coef_ev) HIP_TRY(hipEventCreateWithFlags(&c->air_coef_ev, hipEventDisableTiming));
        c->air_coef_words = total;
    } else if (!rq.d_coefs) {
        HIP_TRY(hipEventSynchronize(c->air_coef_ev)); // the previous upload has left the staging block (long ago, normally)
    }
    const uint64_t *d = c->air_coef_buf;
    *d_rtab = c->air_coef_buf + words;
    if (rq.d_coefs) {
        p.t_alpha = rq.d_coefs; p.t_beta = rq.d_coefs + 115; p.b_alpha = rq.d_coefs + 230; p.b_beta = rq.d_coefs + 230 + na;
        p.a_value = rq.d_avalues ? rq.d_avalues : st.d_static + ((size_t)1 << rq.log_blowup); // null: the AIR's built-in constants
        *d_txl = rq.d_coefs;
        return CSTARK_OK;
    }
    uint64_t *q = c->air_coef_stage;
    memcpy(q, rq.t_alpha, nc * 8); q += nc;
    memcpy(q, rq.t_beta, nc * 8); q += nc;
    memcpy(q, rq.b_alpha, na * 8); q += na;
    memcpy(q, rq.b_beta, na * 8); q += na;
    for (size_t a = 0; a < na; a++) *q++ = s.a_const.empty() ? rq.assertion_values[a] : s.a_const[a];
    memset(q, 0, TXL * 8);
    if (nc <= 115) { memcpy(q, rq.t_alpha, nc * 8); memcpy(q + 115, rq.t_beta, nc * 8); }
    HIP_TRY(hipMemcpyAsync(c->air_coef_buf, c->air_coef_stage, words * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->air_coef_ev, c->stream));
    p.t_alpha = d; p.t_beta = d + nc;
    p.b_alpha = d + 2 * nc; p.b_beta = d + 2 * nc + na; p.a_value = d + 2 * nc + 2 * na;
    *d_txl = d + 2 * nc + 3 * na;
    return CSTARK_OK;
}

// SchnorrAir's transition sum into p.out
int schnorr_transition_sum(cstark_ctx *c, const AirStageRequest &rq, const cs::AirCombineParams &p, const std::vector<uint32_t> &t_grp, const uint64_t *d_txl,
                           uint64_t *d_rtab) {
    const PeriodicTable *pt;
    RC_TRY(get_small_periodic(c, CSTARK_AIR_SCHNORR, 0, rq.log_n, rq.log_blowup, &pt));
    // The doubling / addition gadgets in the degree-split form of the TransactionAir evaluator when the whole extension is at hand
    // (every coset, blowup 8, at least eight signatures): their sums have degree < 4n without the periodic flags, so they are
    // evaluated on the four even cosets, interpolated, extended to the odd cosets and recombined (constraints.hip,
    // k_schnorr_ec_split).  The table must be a genuine extension (rq.own_extension: the prover's own, or what the caller of
    // cstark_schnorr_evaluate_constraints_lde vouches for); cstark_schnorr_evaluate_constraints takes any table and every point
    // directly.  CSTARK_SCHNORR_SPLIT=0: every point directly.
    static const bool split_env = [] { const char *e = getenv("CSTARK_SCHNORR_SPLIT"); return !e || atoi(e) != 0; }();
    if (!(split_env && rq.own_extension && rq.k0 == 0 && rq.nk == 8 && rq.log_blowup == 3 && rq.log_n >= 12 && rq.log_n + 3 <= cs::NTT_MAX_LOG_N && rq.n_items > 1)) {
        HIP_TRY(cs::launch_schnorr_fused(p, rq.d_aux_lde, pt->tab, rq.nk, c->stream));
        return CSTARK_OK;
    }
    // the final addition (degree 5 (n - 1) without its flag) on five cosets: three more tables on the even cosets, LDE coset 1
    // directly (CSTARK_SCHNORR_FINAL5=0: on all eight cosets through the frame evaluator)
    static const bool final5 = [] { const char *e = getenv("CSTARK_SCHNORR_FINAL5"); return !e || atoi(e) != 0; }();
    const unsigned T = final5 ? cs::SCHNORR_SPLIT_TABLES : cs::SCHNORR_SPLIT_EC_TABLES;
    SplitStage st;
    RC_TRY(split_stage(c, rq.log_n, &st));
    const size_t n = st.n, region = (size_t)T * 4 * n, hcol = (size_t)3 * n; // hcol: the final addition's three sums, one n-point table each
    SplitWs w;
    RC_TRY(split_ws_unmerged(c, region, hcol, &w));
    const uint64_t *d_gfold_j;
    RC_TRY(generator_fold_table(c, &d_gfold_j));
    HIP_TRY(cs::launch_schnorr_ec_split(p, rq.d_aux_lde, d_txl, w.even, d_gfold_j, d_rtab + cs::MERKLE_RTAB_LAMBDA, c->stream));
    if (final5) HIP_TRY(cs::launch_schnorr_final_split(p, d_txl, w.even + (size_t)cs::SCHNORR_SPLIT_EC_TABLES * 4 * n, -1, c->stream));
    RC_TRY(inverse_columns(st, w.even, w.sa, w.sb, 4 * T));
    RC_TRY(even_to_odd(st, w.sb, w.sa, T));
    RC_TRY(forward_to_cosets(st, 1, w.sa, w.sc, w.odd, T, (size_t)T * n));
    if (final5) { // the three sums directly on LDE coset 1, then their high parts as for TransactionAir
        HIP_TRY(cs::launch_schnorr_final_split(p, d_txl, w.fin_direct, 1, c->stream));
        RC_TRY(final_hi_unmerged(st, w, 3, cs::SCHNORR_SPLIT_EC_TABLES, 3, cs::SCHNORR_SPLIT_TABLES));
    }
    // the round gadget of the message hash in the folded form (CSTARK_SCHNORR_ROUNDS=0: inside the frame evaluator)
    static const bool rounds_env = [] { const char *e = getenv("CSTARK_SCHNORR_ROUNDS"); return !e || atoi(e) != 0; }();
    HIP_TRY(cs::launch_schnorr_split_finish(p, rq.d_aux_lde, pt->tab, w.even, w.odd, t_grp[0], t_grp[6], c->stream, rounds_env ? d_rtab : nullptr, t_grp[42],
                                            final5 ? w.fin_hi : nullptr));
    return CSTARK_OK;
}

// MerkleAir's transition sum into p.out
int merkle_transition_sum(cstark_ctx *c, const AirStageRequest &rq, const cs::AirCombineParams &p, const std::vector<uint32_t> &t_grp, uint64_t *d_rtab) {
    const PeriodicTable *pt;
    RC_TRY(get_small_periodic(c, CSTARK_AIR_MERKLE_UPDATE, rq.merkle_depth, rq.log_n, rq.log_blowup, &pt));
    // the round gadgets in the folded form of the TransactionAir evaluator (CSTARK_MERKLE_ROUNDS=0: the generic frame evaluator)
    static const bool rounds_env = [] { const char *e = getenv("CSTARK_MERKLE_ROUNDS"); return !e || atoi(e) != 0; }();
    HIP_TRY(cs::launch_merkle_fused(p, pt->tab, rq.nk, c->stream, rounds_env ? d_rtab : nullptr, t_grp[0]));
    return CSTARK_OK;
}

} // namespace

// (internal: declared in ctx.h for the prover)
int air_stage(cstark_ctx *c, const AirStageRequest &rq) {
    cs::host::AirShape s;
    RC_TRY(air_stage_validate(c, rq, s));
    HIP_TRY(hipSetDevice(c->device));
    const cs::AirCombineStatic *st;
    RC_TRY(get_air_static(c, rq, s, &st));
    cs::AirCombineParams p = st->p;
    p.lde = rq.d_lde; p.evals = rq.d_evals; p.out = rq.d_out; p.avals = rq.d_avals_lde; p.n_avals = rq.n_avals; p.k0 = rq.k0;
    const uint64_t *d_txl;
    uint64_t *d_rtab;
    RC_TRY(stage_air_coefs(c, rq, s, *st, p, &d_txl, &d_rtab));
    if (rq.source == AirTransitions::SchnorrFused) RC_TRY(schnorr_transition_sum(c, rq, p, st->t_grp, d_txl, d_rtab));
    if (rq.source == AirTransitions::MerkleFused) RC_TRY(merkle_transition_sum(c, rq, p, st->t_grp, d_rtab));
    if (rq.source != AirTransitions::Materialised) p.tsum = rq.d_out;
    HIP_TRY(cs::launch_air_combine(p, rq.nk, c->stream));
    return CSTARK_OK;
}

extern "C" {

int cstark_air_combine(cstark_ctx *c, int air, uint32_t n_items, const uint64_t *d_lde, const uint64_t *d_evals, const uint64_t *t_alpha,
                       const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta, const uint64_t *assertion_values,
                       const uint64_t *d_avals_lde, uint32_t n_avals, uint64_t *d_out, uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    if (!d_evals) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_combine: null argument");
    AirStageRequest rq;
    rq.air = air; rq.n_items = n_items;
    rq.log_n = log_n; rq.log_blowup = log_blowup; rq.k0 = k0; rq.nk = nk;
    rq.d_lde = d_lde; rq.d_out = d_out;
    rq.source = AirTransitions::Materialised; rq.d_evals = d_evals;
    rq.t_alpha = t_alpha; rq.t_beta = t_beta; rq.b_alpha = b_alpha; rq.b_beta = b_beta; rq.assertion_values = assertion_values;
    rq.d_avals_lde = d_avals_lde; rq.n_avals = n_avals;
    return air_stage(c, rq);
}
int cstark_merkle_evaluate_constraints(cstark_ctx *c, uint32_t merkle_depth, const uint64_t *d_lde, const uint64_t *t_alpha, const uint64_t *t_beta,
                                       const uint64_t *b_alpha, const uint64_t *b_beta, const uint64_t *assertion_values, uint64_t *d_out, uint32_t log_n,
                                       uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    if (merkle_depth > 31) return fail(CSTARK_ERR_INVALID_ARG, "cstark_merkle_evaluate_constraints: unsupported Merkle depth");
    AirStageRequest rq;
    rq.air = CSTARK_AIR_MERKLE_UPDATE;
    rq.log_n = log_n; rq.log_blowup = log_blowup; rq.k0 = k0; rq.nk = nk;
    rq.d_lde = d_lde; rq.d_out = d_out;
    rq.source = AirTransitions::MerkleFused; rq.merkle_depth = merkle_depth;
    rq.t_alpha = t_alpha; rq.t_beta = t_beta; rq.b_alpha = b_alpha; rq.b_beta = b_beta; rq.assertion_values = assertion_values;
    return air_stage(c, rq);
}
// any table: every point directly
int cstark_schnorr_evaluate_constraints(cstark_ctx *c, uint32_t n_sig, const uint64_t *d_lde, const uint64_t *d_aux_lde, const uint64_t *t_alpha,
                                        const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta, const uint64_t *d_avals_lde,
                                        uint32_t n_avals, uint64_t *d_out, uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk) {
    if (!d_aux_lde) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_evaluate_constraints: null argument");
    AirStageRequest rq;
    rq.air = CSTARK_AIR_SCHNORR; rq.n_items = n_sig;
    rq.log_n = log_n; rq.log_blowup = log_blowup; rq.k0 = k0; rq.nk = nk;
    rq.d_lde = d_lde; rq.d_out = d_out;
    rq.source = AirTransitions::SchnorrFused; rq.d_aux_lde = d_aux_lde;
    rq.t_alpha = t_alpha; rq.t_beta = t_beta; rq.b_alpha = b_alpha; rq.b_beta = b_beta;
    rq.d_avals_lde = d_avals_lde; rq.n_avals = n_avals;
    return air_stage(c, rq);
}
// the caller's tables are extensions of columns of degree < n: all eight cosets of blowup 8
int cstark_schnorr_evaluate_constraints_lde(cstark_ctx *c, uint32_t n_sig, const uint64_t *d_lde, const uint64_t *d_aux_lde, const uint64_t *t_alpha,
                                            const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta, const uint64_t *d_avals_lde,
                                            uint32_t n_avals, uint64_t *d_out, uint32_t log_n) {
    if (!d_aux_lde) return fail(CSTARK_ERR_INVALID_ARG, "cstark_schnorr_evaluate_constraints_lde: null argument");
    AirStageRequest rq;
    rq.air = CSTARK_AIR_SCHNORR; rq.n_items = n_sig;
    rq.log_n = log_n; rq.log_blowup = 3; rq.k0 = 0; rq.nk = 8;
    rq.d_lde = d_lde; rq.d_out = d_out;
    rq.source = AirTransitions::SchnorrFused; rq.d_aux_lde = d_aux_lde; rq.own_extension = true;
    rq.t_alpha = t_alpha; rq.t_beta = t_beta; rq.b_alpha = b_alpha; rq.b_beta = b_beta;
    rq.d_avals_lde = d_avals_lde; rq.n_avals = n_avals;
    return air_stage(c, rq);
}

// per-launch timing of the fused constraint evaluation (HIP events on the context's stream)
int cstark_ctx_set_part_timing(cstark_ctx *c, int enable) {
    if (!c) return fail(CSTARK_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (enable && !c->part_ev[0])
        for (hipEvent_t &e : c->part_ev) HIP_TRY(hipEventCreate(&e));
    c->part_timing = enable != 0;
    c->part_valid = false;
    return CSTARK_OK;
}
int cstark_lde_timing_ms(cstark_ctx *c, float *total_ms, uint64_t *elements) {
    if (!c || !total_ms || !elements) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    float sum = 0;
    if (c->lde_ev_used) HIP_TRY(hipEventSynchronize(c->lde_ev[c->lde_ev_used - 1]));
    for (size_t i = 0; i + 1 < c->lde_ev_used; i += 2) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->lde_ev[i], c->lde_ev[i + 1]));
        sum += ms;
    }
    *total_ms = sum;
    *elements = c->lde_units;
    c->lde_ev_used = 0;
    c->lde_units = 0;
    return CSTARK_OK;
}
int cstark_tx_constraint_part_ms(cstark_ctx *c, float *ms /* [9] */) {
    if (!c || !ms) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    if (!c->part_valid) return fail(CSTARK_ERR_INVALID_ARG, "no timed constraint evaluation has run (cstark_ctx_set_part_timing)");
    HIP_TRY(hipEventSynchronize(c->part_ev[cs::CE_NUM_PARTS]));
    for (int i = 0; i < cs::CE_NUM_PARTS; i++) HIP_TRY(hipEventElapsedTime(&ms[i], c->part_ev[i], c->part_ev[i + 1]));
    return CSTARK_OK;
}

// host-side view of the AIR description, for the CPU tests
int cstark_tx_constraint_degree(uint32_t i, uint32_t *base, uint32_t *cycles) {
    if (i >= CSTARK_TX_NUM_CONSTRAINTS || !base || !cycles) return fail(CSTARK_ERR_INVALID_ARG, "constraint index out of range");
    const int g = cs::tx_degree_group((int)i);
    *base = cs::TX_GROUP_BASE[g];
    *cycles = cs::TX_GROUP_CYCLES[g];
    return CSTARK_OK;
}
int cstark_tx_periodic_columns(uint32_t merkle_depth, uint64_t *out /* [48][1024] host */) {
    std::vector<uint64_t> cols;
    if (!out || !cs::host::tx_periodic_columns(merkle_depth, cols)) return fail(CSTARK_ERR_INVALID_ARG, "unsupported Merkle depth");
    memcpy(out, cols.data(), cols.size() * 8);
    return CSTARK_OK;
}

// ---- trace validation ----------------------------------------------------------------------------------------------
// the raw periodic columns of (air, depth) on the device, uploaded on first use and kept with the context
static int get_raw_periodic(cstark_ctx *c, int air, unsigned depth, const cs::host::TraceCheckShape &s, const uint64_t **out) {
    *out = nullptr;
    if (s.n_per == 0) return CSTARK_OK;
    for (const cs::RawPeriodic &t : c->raw_periodic)
        if (t.air == air && t.depth == depth) { *out = t.tab; return CSTARK_OK; }
    std::vector<uint64_t> cols;
    bool ok = true;
    if (air == CSTARK_AIR_STATE_TRANSITION) ok = cs::host::tx_periodic_columns(depth, cols);
    else if (air == CSTARK_AIR_MERKLE_UPDATE) ok = cs::host::merkle_periodic_columns(depth, cols);
    else if (air == CSTARK_AIR_SCHNORR) cs::host::schnorr_mask_columns(cols);
    else cs::host::rescue_chain_periodic_columns(cols);
    if (!ok || cols.size() != ((size_t)s.n_per << s.log_cycle)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: unsupported Merkle depth");
    cs::RawPeriodic t{air, depth, nullptr};
    DevGuard g;
    HIP_TRY(g.alloc(&t.tab, cols.size() * 8));
    HIP_TRY(hipMemcpyAsync(t.tab, cols.data(), cols.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->raw_periodic.push_back(t);
    g.release();
    *out = t.tab;
    return CSTARK_OK;
}
int cstark_air_trace_shape(int air, uint32_t log_n, uint32_t *width, uint32_t *n_constraints, uint32_t *log_cycle) {
    cs::host::TraceCheckShape s;
    if (!width || !n_constraints || !log_cycle || !cs::host::trace_check_shape(air, log_n, s))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_trace_shape: not an AIR, or a trace length it cannot have");
    *width = s.width; *n_constraints = s.nc; *log_cycle = s.log_cycle;
    return CSTARK_OK;
}
int cstark_air_validate_trace(cstark_ctx *c, int air, const uint64_t *d_trace, uint32_t log_n, uint32_t item, const uint64_t *public_inputs,
                              cstark_trace_report *report, uint32_t *cycle_codes, uint64_t *frame_values) {
    if (!c || !d_trace || !report) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: null argument");
    cs::host::TraceCheckShape s;
    if (air < CSTARK_AIR_STATE_TRANSITION || air > CSTARK_AIR_RESCUE_CHAIN) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: unknown AIR");
    if (!cs::host::trace_check_shape(air, log_n, s))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: the AIR has no trace of this length (at least one cycle, at most 2^24 rows)");
    const bool tree = air == CSTARK_AIR_STATE_TRANSITION || air == CSTARK_AIR_MERKLE_UPDATE;
    if (tree && !cs::host::trace_check_depth(item)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: the Merkle depth must be 1, 3, 7, 15 or 31");
    const unsigned depth = tree ? item : 0;
    const size_t n = (size_t)1 << log_n, n_cycles = n >> s.log_cycle;
    const unsigned n_pub = air == CSTARK_AIR_SCHNORR ? 0 : air == CSTARK_AIR_RANGE ? 1 : 14;
    if (public_inputs)
        for (unsigned i = 0; i < n_pub; i++)
            if (public_inputs[i] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: a public input is not a reduced field element");
    size_t n_sig = 0;
    if (air == CSTARK_AIR_SCHNORR) {
        n_sig = c->schnorr_rx.size() / 6;
        if (n_sig == 0 || n_sig * 512 != n || c->schnorr_pub.size() < n_sig * 28)
            return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: no Schnorr statement uploaded for this trace length");
    }
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t *d_per;
    RC_TRY(get_raw_periodic(c, air, depth, s, &d_per));
    std::vector<cs::ValidateEntry> entries;
    std::vector<uint64_t> seq;
    if (public_inputs && !cs::host::trace_check_entries(air, log_n, public_inputs, c->schnorr_rx.data(), entries, seq))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_validate_trace: no boundary list for this AIR");
    // scratch of the call: codes [n_cycles] | summary [4] (32-bit words), then 64-bit words: messages | sequences | boundary list | one frame
    // (cur, next, periodic values, public-input values, slot values).  At 2^24 rows: 8 MiB of codes (RescueAir), or 7 MiB + 3 MiB of statement words (SchnorrAir); below 64 MiB whatever the AIR and n.
    const size_t code_words = (n_cycles + 4 + 1) & ~(size_t)1;
    const size_t msg_words = n_sig * 28, ent_words = entries.size() * sizeof(cs::ValidateEntry) / 8;
    const size_t frame_in = 2 * (size_t)s.width + s.n_per + 19, frame_words = frame_in + s.nc;
    const size_t stage_words = msg_words + seq.size() + ent_words, bytes = code_words * 4 + (stage_words + frame_words) * 8;
    static_assert(sizeof(cs::ValidateEntry) == 24, "boundary entries are staged as three words each");
    if (c->val_bytes < bytes) {
        if (c->val_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->val_buf)); c->val_buf = nullptr; c->val_bytes = 0; }
        HIP_TRY(hipMalloc(&c->val_buf, bytes));
        c->val_bytes = bytes;
    }
    uint32_t *d_codes = (uint32_t *)c->val_buf, *d_summary = d_codes + n_cycles;
    uint64_t *d_stage = (uint64_t *)(d_codes + code_words), *d_frame = d_stage + stage_words;
    std::vector<uint64_t> stage(stage_words);
    if (msg_words) memcpy(stage.data(), c->schnorr_pub.data(), msg_words * 8);
    if (!seq.empty()) memcpy(stage.data() + msg_words, seq.data(), seq.size() * 8);
    if (ent_words) memcpy(stage.data() + msg_words + seq.size(), entries.data(), ent_words * 8);
    HIP_TRY(hipMemsetAsync(d_codes, 0xFF, (n_cycles + 2) * 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_summary + 2, 0, 8, c->stream));
    if (stage_words) HIP_TRY(hipMemcpyAsync(d_stage, stage.data(), stage_words * 8, hipMemcpyHostToDevice, c->stream));
    cs::ValidateParams p{};
    p.trace = d_trace; p.per = d_per; p.messages = msg_words ? d_stage : nullptr;
    p.codes = d_codes; p.summary = d_summary; p.log_n = log_n; p.log_cycle = s.log_cycle;
    hipError_t e = cs::launch_validate_frames(air, p, c->stream);
    if (e == hipSuccess && !entries.empty())
        e = cs::launch_validate_boundary(p, (const cs::ValidateEntry *)(d_stage + msg_words + seq.size()), (unsigned)entries.size(),
                                         seq.empty() ? nullptr : d_stage + msg_words, n_sig ? (unsigned)n_sig : 1u, c->stream);
    uint32_t summary[4];
    if (e == hipSuccess) e = hipMemcpyAsync(summary, d_summary, sizeof summary, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream); // also: `stage` is no longer read
    HIP_TRY(e);
    HIP_TRY(e_sync);
    cstark_trace_report rep{};
    rep.step = -1; rep.constraint = CSTARK_TRACE_CLEAN; rep.bad_cycles = summary[2]; rep.boundary = -1;
    if (summary[1] != cs::VALIDATE_CLEAN) {
        rep.boundary = (int32_t)(summary[1] >> 24);
        rep.boundary_register = entries[rep.boundary].reg;
        rep.boundary_step = summary[1] & 0xFFFFFFu;
    }
    std::vector<uint64_t> values;
    if (summary[0] != cs::VALIDATE_CLEAN) {
        uint32_t code;
        HIP_TRY(hipMemcpyAsync(&code, d_codes + summary[0], 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const cs::host::TraceViolation v = cs::host::trace_check_decode(s, summary[0], code);
        rep.step = (int64_t)v.step; rep.constraint = v.constraint;
        // every slot of that one frame through the free-standing-frame kernels: the caller's frame_values, and the two evaluators' cross-check
        HIP_TRY(cs::launch_validate_gather_frame(p, d_frame, (size_t)v.step, s.width, s.n_per, c->stream));
        HIP_TRY(cs::launch_eval_frames_air(air, d_frame, d_frame + s.width, d_frame + 2 * s.width, d_frame + frame_in, 1, c->stream));
        values.resize(s.nc);
        HIP_TRY(hipMemcpyAsync(values.data(), d_frame + frame_in, (size_t)s.nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (values[v.constraint] == 0)
            return fail(CSTARK_ERR_HIP, "cstark_air_validate_trace: the two evaluators disagree (the frame kernel names a constraint whose value on that frame is zero)");
    }
    if (cycle_codes) {
        HIP_TRY(hipMemcpyAsync(cycle_codes, d_codes, n_cycles * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (frame_values && !values.empty()) memcpy(frame_values, values.data(), values.size() * 8);
    *report = rep;
    return CSTARK_OK;
}

} // extern "C"
