/*
 * gigapose_dist.h -- C-ABI of libgigapose_dist.so: all-pairs vertex distances on MI355X (gfx950).  Two things a user of a pose
 * estimator expects beside the BOP-19 errors of gigapose_eval.h: ADD and ADD-S (Hinterstoisser et al., ACCV 2012: the mean
 * distance of the model's vertices under the estimate to the same / to the nearest vertex under the ground truth -- the numbers
 * LM, LM-O and YCB-V tables are written in), and the model diameter every threshold is a multiple of (bop_toolkit: the largest
 * distance between two vertices), for a mesh that comes without a models_info.json.  ADD-S and the diameter are O(V^2) per
 * item.  The definitions below ARE the contract: no toolkit is consulted.  This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_eval.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpd_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Limits: N <= 65535 per call (the grid's second dimension; gigapose_amd/distances.py chunks the pairs), 1 <= V <= 2^20,
 * -64 <= k <= 64, n < 2^31.  The calls initialise their outputs.  N = 0 (n = 0) is a no-op that returns 0.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/dist_ref.py restates it in numpy and must agree bit for bit).  All
 * floating-point work is IEEE float64, one rounding per written operation, in the written order, no contraction (the library
 * is built with -ffp-contract=off) -- with ONE exception, the fused operation of the square root below.  Maxima, minima and
 * sums are taken over INTEGERS or are exact (a minimum or maximum of doubles none of which is a NaN), so no result depends on
 * how the work is spread over threads, waves and workgroups, or on the order in which they finish.
 *
 * The square root.  root(x) is the CORRECTLY ROUNDED float64 square root (what numpy.sqrt returns).  Whether the compiler's
 * expansion of a float64 sqrt for gfx950 is correctly rounded is documented nowhere, so the library does not rest on it: for
 * 0 < x < +inf it takes the compiler's root r (within one unit in the last place), its neighbours r- and r+ (the adjacent
 * doubles), and decides with two FUSED multiply-adds -- explicit fma() calls, which stay fused under -ffp-contract=off and are
 * the one fused operation of the library:
 *     if fma(r-, r, -x) >= 0: root = r-;   else if fma(r, r+, -x) < 0: root = r+;   else root = r
 * Why that is exact: sqrt(x) lies below the midpoint of two adjacent doubles a < b = a + h iff x < (a + h/2)^2 = a*b + h*h/4.
 * With a = m * h, a*b is a multiple of h*h, and so is x (x ~ a*a has an exponent about 52 above h*h's and 53 bits); no
 * multiple of h*h lies strictly between a*b and a*b + h*h/4, so the condition is x <= a*b, and the sign of fma(a, b, -x) --
 * one rounding of the exact a*b - x, which keeps the sign and an exact zero -- decides it.  (At x = a*b the root is the
 * geometric mean, below the midpoint: it rounds to a.)  So that a*b - x cannot underflow, an x below 2^-500 is multiplied by
 * 2^512 first and its root by 2^-256 afterwards; both are exact.  0, -0, +inf, a NaN and a negative x give what sqrt gives.
 */
#ifndef GIGAPOSE_DIST_H
#define GIGAPOSE_DIST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpd_abi_version(void);
const char* gpd_last_error(void);

/* ADD.  vertices (V,3) f32; est, gt (N,4,4) f64, object -> camera, row-major, rows 0..2 are read, in the units of the
 * vertices  ->  sums (N) int64, 8-byte aligned; status (N) int32.
 * For pair n and vertex i = (x, y, z) converted to float64, with P = est[n], G = gt[n]:
 *     eX = ((P00*x + P01*y) + P02*z) + P03    eY, eZ likewise from rows 1, 2;   gX, gY, gZ likewise from G
 *     d2(a, b) = ((aX-bX)*(aX-bX) + (aY-bY)*(aY-bY)) + (aZ-bZ)*(aZ-bZ)
 *     v_i = d2(e_i, g_i)
 *     r_i = root(v_i)                       the correctly rounded root, see above
 *     s_i = r_i * 2^k                       exact
 *     q_i = (int64) rint(s_i)               half to even;  q_i = 0 if s_i is not below 2^42
 *     sums[n] = sum over i of q_i           an INTEGER sum
 * (q_i rounds the ROUNDED root: it differs from the half-to-even rounding of the exact sqrt(v_i) * 2^k only where that lies
 * within a relative 2^-53 of the middle between two integers.)
 * The caller's error is sums[n] / (V * 2^k): the mean distance in quanta of 2^-k units (k = 20 and millimetres: about 1e-6 mm
 * of resolution, distances up to 2^22 mm).
 * status[n], bit 0: a coordinate of e or g of this pair is not finite, or some v_i is not below +inf;
 *            bit 1: some s_i is not below 2^42 (a NaN is not below anything).  With V <= 2^20 a sum stays below 2^62.
 * A pair with a status bit set has a sum that means nothing: the caller reports +inf for it. */
int gpd_add(const float* vertices, int V, const double* est, const double* gt, int N, int k, long long* sums, int* status,
            void* stream);

/* ADD-S: the same with
 *     v_i = min over j in [0, V) of d2(g_i, e_j)
 * -- for each GROUND-TRUTH point the nearest ESTIMATE point (Hinterstoisser's definition, bop_toolkit's adi); the other
 * direction is a different number.  The minimum starts at +inf and takes a candidate c where c < m: a NaN candidate is never
 * taken (numpy.fmin), and with finite coordinates there is none, so the minimum is exact and independent of the order. */
int gpd_adds(const float* vertices, int V, const double* est, const double* gt, int N, int k, long long* sums, int* status,
             void* stream);

/* The square of the model diameter.  vertices (V,3) f32  ->  key (1) u64, 8-byte aligned: the bit pattern of
 *     max over all i < j of d2(vertex_i, vertex_j)
 * of the float64 conversions of the f32 coordinates, the same expression (bit patterns of non-negative doubles order like the
 * doubles: the maximum is merged with a 64-bit unsigned atomic maximum).  A d2 that is not below +inf takes the key of all
 * ones -- with V >= 2 that is the case exactly when some coordinate is not finite, since squares of f32 differences cannot
 * overflow a double.  V = 1 has no pair: the key is 0.  The caller takes the root on the host. */
int gpd_diameter2(const float* vertices, int V, unsigned long long* key, void* stream);

/* out[i] = root(x[i]), i < n: the library's square root on its own, so that its rounding can be tested. */
int gpd_root(const double* x, long long n, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_DIST_H */
