/* cstark_debug_ood.h -- TEST-ONLY, served by libcstark_debug.so like cstark_debug_ntt.h: this entry point drives internal functions of
 * the product library (csrc/ctx.h), which is why it is declared apart from cstark_debug.h.
 * Field elements: uint64_t in BaseElement memory form; an element of the degree-m extension is m consecutive words.  Return: cstark_status.
 */
#ifndef CSTARK_DEBUG_OOD_H
#define CSTARK_DEBUG_OOD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The out-of-domain frame and the quotient sums of the DEEP composition as the prover computes them when its channel runs on the
 * device (csrc/prove.hip): every point, coefficient and frame value is read from device memory.  m = 1, 2, 3; `ctx` is a cstark_ctx.
 * All pointers are device memory:
 *   d_pts       z | z w | z^n_comp, m-tuples (3 m words)
 *   d_coeffs    [width][n] coefficient columns; d_ccoef [m n_comp][n] (column m i + q = component q of composition column i)
 *   d_trace_lde [nk..][width][n], d_comp_lde [nk..][m n_comp][n]: the first nk cosets are read
 *   d_coef      alpha[width] | beta[width] | delta[n_comp], m-tuples
 *   d_deg       deg_a | deg_b, m-tuples
 *   d_shifts    [2^log_blowup] coset offsets g w_(b n)^k
 *   d_ood_in    null: the DEEP stage reads the frame computed here; else a frame of the same layout to read instead
 *   d_scal      8 m words of scratch (z | z w | z^n_comp | deg_a | deg_b | k1 | k2 | k3 as the kernels read them)
 *   d_frame     out: T(z)[width] | T(z w)[width] | H_i(z^n_comp)[n_comp], m-tuples
 *   d_sums      out: m = 1: [nk][n]; m > 1: [m][nk][n]
 * Runs ood_frames_dev / ood_frames_dev_ext, then k_deep with its device scalars (m = 1) or deep_composition_ext_dev; synchronises
 * the context's stream. */
int cstark_debug_ood_deep_dev(void *ctx, uint32_t m, const uint64_t *d_pts, const uint64_t *d_coeffs, uint32_t width, const uint64_t *d_ccoef,
                              uint32_t n_comp, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, const uint64_t *d_coef, const uint64_t *d_deg,
                              const uint64_t *d_shifts, const uint64_t *d_ood_in, uint64_t *d_scal, uint32_t nk, uint32_t log_n, uint32_t log_blowup,
                              uint64_t *d_frame, uint64_t *d_sums);
#ifdef __cplusplus
}
#endif
#endif
