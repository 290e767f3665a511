/* cstark_debug_ntt.h -- TEST-ONLY, served by libcstark_debug.so like cstark_debug.h.  Unlike the element-wise operations there, this
 * entry point drives kernels of the product library (libcstark_debug.so links to libcstark_hip.so), which is why it is declared apart.
 * Field elements: uint64_t in BaseElement memory form; `stream` is a hipStream_t.  Return: cstark_status.
 */
#ifndef CSTARK_DEBUG_NTT_H
#define CSTARK_DEBUG_NTT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The extension of polynomials of degree < 4n from the four even cosets of the 8n-point domain to the four odd ones, plain and merged
 * (csrc/ntt.h).  d_in = [4 tables][4 even cosets][n] interpolants (device); d_plain = [4 odd cosets][4 tables][n]: coset_even_to_odd;
 * d_merged = [4 odd cosets][2][n]: coset_even_to_odd_merged for the families S_0 + x^e[0] S_1 + x^e[1] S_2 and x^e[2] S_3, with
 * x = LDE offset * y.  e: three host words, any exponents.  2^8 <= n; synchronises the stream. */
int cstark_debug_split_merge(void *stream, const uint64_t *d_in, uint64_t *d_plain, uint64_t *d_merged, uint32_t log_n, const uint64_t *e);
#ifdef __cplusplus
}
#endif
#endif
