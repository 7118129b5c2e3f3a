/*
 * gigapose_eval.h -- C-ABI of libgigapose_eval.so: scoring pose estimates against ground truth on MI355X (gfx950), the stage
 * behind the BOP csv files gigapose_amd/inout.py writes.  The reference shells out to bop_toolkit's eval_bop19_pose.py with
 * --renderer_type=vispy (src/scripts/eval_bop.py:29), which needs an OpenGL context; an Instinct accelerator has none.  This
 * library computes the three BOP-19 pose errors (Hodan et al., "BOP Challenge 2020", section 2.2): MSSD and MSPD -- the
 * maximum surface / projection deviation over the model's vertices, minimised over its symmetry transforms -- and VSD, from
 * the depth maps libgigapose_render.so draws.  The definitions below ARE the contract: bop_toolkit is not consulted.
 * This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_render.h)
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all buffers, kernels never allocate;
 *     inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpe_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Limits: N <= 65535 per call (the grid's second dimension; gigapose_amd/evaluate.py chunks the pairs), H*W < 2^31,
 * V >= 1, S >= 1, T <= GPE_MAX_THRESHOLDS; every buffer is addressed through size_t (N*H*W passes 2^31 elements at 6 991
 * depth maps of 480 x 640).
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/eval_ref.py restates it in numpy and must agree bit for bit).  All
 * floating-point work is IEEE float64, one rounding per written operation, in the written order, no fused multiply-add (the
 * library is built with -ffp-contract=off); float64 division is the correctly rounded one (see gigapose_render.h).  Maxima,
 * minima and sums are taken over INTEGERS (the bit patterns of non-negative doubles order like the doubles; counts), so no
 * result depends on how the work is spread over threads, waves and workgroups, or on the order in which they finish.
 */
#ifndef GIGAPOSE_EVAL_H
#define GIGAPOSE_EVAL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpe_abi_version(void);
const char* gpe_last_error(void);

/* Bytes of the workspace gpe_mssd_mspd needs for N pairs and S symmetry transforms: per (pair, symmetry) the 12 doubles of
 * gt * sym and two 8-byte keys.  0 if an argument is negative. */
size_t gpe_pose_workspace_bytes(int N, int S);

/* vertices (V,3) f32; syms (S,4,4) f64, row-major, syms[0] = identity (not checked; rows 0..2 are read, the last row is taken
 * as 0, 0, 0, 1); est, gt (N,4,4) f64, object -> camera, row-major, rows 0..2 are read, in the units of the vertices; K (N,9)
 * f64, one camera per pair, entries 0..5 are read; zmin f64, finite  ->  mssd2 (N) f64, mspd2 (N) f64: the SQUARED errors (the
 * caller takes the roots: the bits never rest on a device sqrt).
 * For pair n, symmetry s, vertex (x, y, z) converted to float64, with g = gt[n], S = syms[s], P = est[n], K = K[n]:
 *     G_ij = (g_i0*S_0j + g_i1*S_1j) + g_i2*S_2j          j = 0, 1, 2
 *     G_i3 = ((g_i0*S_03 + g_i1*S_13) + g_i2*S_23) + g_i3
 *     eX = ((P00*x + P01*y) + P02*z) + P03    eY, eZ likewise from rows 1, 2;   gX, gY, gZ likewise from G
 *     d2 = ((eX-gX)*(eX-gX) + (eY-gY)*(eY-gY)) + (eZ-gZ)*(eZ-gZ)
 *     eu = ((K0*eX + K1*eY) + K2*eZ) / eZ     ev = ((K3*eX + K4*eY) + K5*eZ) / eZ     gu, gv likewise from gX, gY, gZ
 *     p2 = (eu-gu)*(eu-gu) + (ev-gv)*(ev-gv)
 *     mssd2[n] = min over s of max over vertices of d2        mspd2[n] = min over s of max over vertices of p2
 * Bad inputs: if ANY d2 of the pair (any s, any vertex) is not finite, mssd2[n] = +inf; if any p2 is not finite, or any eZ or
 * gZ is below zmin, mspd2[n] = +inf.  A NaN is never dropped by a comparison: a value that is not below +inf takes the key
 * of all ones, the keys are compared as unsigned integers, and a key of all ones anywhere in the pair gives +inf.
 *
 * Rounding error against the exact value for the float64 inputs (tests/test_eval_host.py holds the restatement to it), with
 * u = 2^-53 and gamma_k = k*u / (1 - k*u), gamma_a + gamma_b + gamma_a*gamma_b <= gamma_(a+b):
 *   - a coordinate of e is a 4-term dot product: 3 products, 3 sums, at most 4 roundings on any term: error <= gamma_4 * Be,
 *     Be = max_i (|P_i0||x| + |P_i1||y| + |P_i2||z| + |P_i3|);
 *   - an entry of G carries gamma_4 the same way, a coordinate of g then gamma_4 more: error <= gamma_8 * Bg,
 *     Bg = max_i sum_j (sum_k |g_ik||S_kj|) |x_j| (with x_3 = 1, |g_i3| added for j = 3);
 *   - a difference adds one rounding: with B = Be + Bg (a bound of every difference), error of a difference <= eps = gamma_9 * B;
 *   - d2 is 3 products and 2 sums, gamma_3 on the computed squares:
 *         |d2 - exact| <= 3*B*B * (2*gamma_9 + gamma_9^2 + gamma_3*(1 + gamma_9)^2)
 *   - the numerator of a projection is a 3-term dot product of coordinates that carry gamma_8: error <= gamma_11 * Bn with
 *     Bn = max(|K0|+|K1|+|K2|, |K3|+|K4|+|K5|) * max(Be, Bg); dividing by a Z with |Z| >= Zlow > 0 (exact and computed) and
 *     rounding once: with U = Bn / Zlow and rho = max(Be, Bg) / Zlow, error of u, v <= eta = U * (gamma_12 + gamma_8 * rho);
 *   - a pixel difference is bounded by D = 2*U and carries eps_p = 2*eta + u*D <= 2*U*(gamma_13 + gamma_8*rho); p2 is 2
 *     products and 1 sum:
 *         |p2 - exact| <= 2*(2*D*eps_p + eps_p^2) + gamma_2 * 2 * (D + eps_p)^2
 *   - maximum and minimum are exact and do not grow a bound: the bounds hold for mssd2 and mspd2 with the largest B, U, rho of
 *     the pair.
 * workspace: gpe_pose_workspace_bytes(N, S) bytes, 8-byte aligned; the call initialises it. */
int gpe_mssd_mspd(const float* vertices, int V, const double* syms, int S, const double* est, const double* gt, const double* K,
                  int N, double zmin, double* mssd2, double* mspd2, void* workspace, void* stream);

#define GPE_MAX_THRESHOLDS 16

/* Visible surface discrepancy as integer counts.  depth_est, depth_gt (N,H,W) f32: z-depths as gpr_resolve writes them, 0 =
 * nothing drawn; depth_test (M,H,W) f32: the sensor's z-depth in the same units, 0 = no measurement; frame (N) int32 into M;
 * ray (R,H,W) f64: the length of the viewing ray through each pixel at unit depth, computed by the caller on the host as
 * sqrt((a*a + b*b) + 1.0) with a = (px - K2) / K0, b = (py - K5) / K4; ray_index (N) int32 into R; delta f64; thr (N,T) f64
 * (tau_t * diameter_n, computed by the caller), 1 <= T <= GPE_MAX_THRESHOLDS
 *   ->  counts (N, 2+T) int64 = union, intersection, bad[0..T-1].  The call initialises counts.
 * Per pixel, with de, dg, dt the three depths there (a depth that is negative, NaN or infinite counts as 0):
 *     De = (double)de * ray    Dg = (double)dg * ray    Dt = (double)dt * ray
 *     visible(m) = (dm > 0 && dt > 0 && (Dm - Dt) <= delta) || (dm > 0 && dt == 0)               [the BOP-19 visibility]
 *     vis_gt = visible(g)      vis_est = visible(e) || (vis_gt && de > 0)
 *     union += vis_gt || vis_est        intersection += vis_gt && vis_est
 *     at an intersection pixel: cost = |Dg - De|; bad[t] += cost >= thr[n][t]
 * The caller's error is e_t = (bad[t] + union - intersection) / union, or 1.0 when union = 0.
 * A pair whose frame or ray_index lies outside [0, M) / [0, R) reads nothing: its union is -1 and the rest 0. */
int gpe_vsd_counts(const float* depth_est, const float* depth_gt, int N, const float* depth_test, int M, const int* frame,
                   const double* ray, int R, const int* ray_index, int H, int W, double delta, const double* thr, int T,
                   long long* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_EVAL_H */
