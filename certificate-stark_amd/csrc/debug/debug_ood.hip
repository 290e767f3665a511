// The device-channel forms of the out-of-domain frame and the DEEP quotient sums, reachable from a test (include/cstark_debug_ood.h):
// the functions of ctx.h that prove.hip calls after the device channel drew the point, in its order and with its scratch handling.
#include <hip/hip_runtime.h>
#include "../../../include/cstark_debug_ood.h"
#include "../ctx.h"
#include "../deep.h"
#include "../ntt.h"

extern "C" int cstark_debug_ood_deep_dev(void *ctx, uint32_t m, const uint64_t *d_pts, const uint64_t *d_coeffs, uint32_t width, const uint64_t *d_ccoef,
                                         uint32_t n_comp, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, const uint64_t *d_coef,
                                         const uint64_t *d_deg, const uint64_t *d_shifts, const uint64_t *d_ood_in, uint64_t *d_scal, uint32_t nk,
                                         uint32_t log_n, uint32_t log_blowup, uint64_t *d_frame, uint64_t *d_sums) {
    cstark_ctx *c = (cstark_ctx *)ctx;
    if (!c || !d_pts || !d_coeffs || !d_ccoef || !d_trace_lde || !d_comp_lde || !d_coef || !d_deg || !d_shifts || !d_scal || !d_frame || !d_sums)
        return CSTARK_ERR_INVALID_ARG;
    if (m < 1 || m > 3 || width == 0 || n_comp == 0 || log_n < cs::NTT_MIN_LOG_N || log_n > cs::NTT_MAX_LOG_N || log_blowup > 6 || nk == 0 ||
        nk > (1u << log_blowup))
        return CSTARK_ERR_INVALID_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CSTARK_ERR_HIP;
    hipStream_t st = c->stream;
    // the frame: the scratch is reserved ahead of the launches, as the prover does
    RC_TRY(desc_reserve(c, ood_frames_dev_scratch_bytes(width, n_comp, log_n, m)));
    if (m == 1) RC_TRY(ood_frames_dev(c, d_coeffs, width, d_ccoef, n_comp, log_n, d_pts, d_frame));
    else RC_TRY(ood_frames_dev_ext(c, d_coeffs, width, d_ccoef, n_comp, log_n, m, d_pts, d_frame));
    // where the channel leaves the points and the degree adjustments: z | z w | z^n_comp | deg_a | deg_b
    if (hipMemcpyAsync(d_scal, d_pts, (size_t)3 * m * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return CSTARK_ERR_HIP;
    if (hipMemcpyAsync(d_scal + 3 * m, d_deg, (size_t)2 * m * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return CSTARK_ERR_HIP;
    const uint64_t *d_ood = d_ood_in ? d_ood_in : d_frame;
    if (m == 1) {
        const uint64_t *pw, *pwinv;
        RC_TRY(plan_tables(c, log_n, &pw, &pwinv));
        cs::DeepParams p{};
        p.trace_lde = d_trace_lde; p.comp_lde = d_comp_lde; p.w = pw; p.coef = d_coef; p.ood = d_ood; p.shifts = d_shifts; p.out = d_sums;
        p.width = width; p.nb = n_comp; p.log_n = log_n; p.k0 = 0; p.scal = d_scal;
        if (cs::deep_composition(p, nk, st) != hipSuccess) return CSTARK_ERR_HIP;
    } else {
        RC_TRY(deep_composition_ext_dev(c, d_trace_lde, d_comp_lde, width, n_comp, m, d_coef, d_ood, d_scal, d_shifts, d_sums, log_n, log_blowup, nk));
    }
    return hipStreamSynchronize(st) == hipSuccess ? CSTARK_OK : CSTARK_ERR_HIP;
}
