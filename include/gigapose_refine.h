/*
 * gigapose_refine.h -- C-ABI of libgigapose_refine.so: refining pose estimates against the sensor's depth image on MI355X
 * (gfx950), the stage behind the coarse pose.  Point-to-plane ICP with same-pixel (projective) association: the estimate is
 * drawn by libgigapose_render.so (gpr_project + gpr_raster: a z-buffer of 64-bit keys), every covered pixel whose measured
 * depth lies within a gate of the drawn depth contributes one row to the Gauss-Newton normal equations of a small rigid motion
 * (gpf_accumulate, the hot kernel), and the motion that solves them is applied to the pose (gpf_update).  Reference: the role
 * of ICPRefiner.refine_poses (src/megapose/inference/icp_refiner.py: render, compare with the measured depth, move the pose,
 * keep the input pose when the fit fails); nothing of it or of the ICP it calls is restated, the definitions below ARE the
 * contract.  This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_eval.h and gigapose_dist.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpf_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Limits: N <= 65535 per call (the grid's second dimension; gigapose_amd/refine.py chunks the pairs), H*W <= 2^22 (the bound
 * on an integer sum below), 0 <= F < 2^31, 1 <= V < 2^31, M >= 1; every buffer is addressed through size_t (the key buffer
 * passes 2^31 elements at 874 pairs of 480 x 640).  N = 0 (F = 0 for gpf_face_normals) is a no-op that returns 0.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/refine_ref.py restates it in numpy and must agree bit for bit).  All
 * floating-point work is IEEE float64, one rounding per written operation, in the written order, no fused multiply-add (the
 * library is built with -ffp-contract=off); `/` is the correctly rounded float64 division (gigapose_render.h says why the
 * build gives it).  There is no square root and no transcendental function anywhere on the device: the weight 1/(m.m) stands
 * for the normalisation of the normal, and the rotation is formed by the Cayley transform, which is rational.  Per-pixel terms
 * are quantised BEFORE they are summed and only INTEGERS are merged, so no result depends on how the pixels are spread over
 * threads, waves and workgroups, or on the order in which they finish.
 */
#ifndef GIGAPOSE_REFINE_H
#define GIGAPOSE_REFINE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpf_abi_version(void);
const char* gpf_last_error(void);

/* Layout of one pair's row of sums: 32 int64 = 256 bytes.
 *   [0, 21)  w g_i g_j for i <= j, row by row: 00 01 02 03 04 05 11 12 13 14 15 22 23 24 25 33 34 35 44 45 55
 *   [21, 27) w g_i e        27  w e e        28  covered        29  count        30, 31  padding, always 0 */
#define GPF_SUMS 32
#define GPF_SUM_RHS 21
#define GPF_SUM_EE 27
#define GPF_SUM_COVERED 28
#define GPF_SUM_COUNT 29
#define GPF_QUANTUM_BITS 36 /* a term is added as rint(term * 2^36) */
#define GPF_TERM_MAX 16.0   /* a pixel with y.y or a squared term above this is dropped */

/* status (gpf_accumulate) */
#define GPF_RANGE 1     /* a pixel that passed the gate was dropped: y.y or a squared term is not <= GPF_TERM_MAX */
#define GPF_BAD_INDEX 2 /* a covered pixel names a face >= F or a face whose m.m is a NaN or +inf; or frame[n] lies outside [0, M) */
/* state (gpf_update); the first three are the STOP bits */
#define GPF_FEW 4         /* count < min_points */
#define GPF_DEGENERATE 8  /* a pivot is not above min_pivot * count, or the step is not finite */
#define GPF_CLIPPED 16    /* the view dropped a triangle (clipped[n] != 0) */
#define GPF_CONVERGED 32  /* the last step had xi.xi < tol2; reported, does not stop the pair */
#define GPF_STOP (GPF_FEW | GPF_DEGENERATE | GPF_CLIPPED)

/* vertices (V,3) f32, faces (F,3) int32 -> c (F,3) f64: the UNNORMALISED normal of each face in model coordinates.  With the
 * face's vertices p0, p1, p2 converted to float64:
 *     u = p1 - p0,  v = p2 - p0   (component by component)
 *     c = (u1*v2 - u2*v1,  u2*v0 - u0*v2,  u0*v1 - u1*v0)
 * A vertex index outside [0, V) gives c = (NaN, NaN, NaN).  Runs once per mesh. */
int gpf_face_normals(const float* vertices, int V, const int* faces, int F, double* c, void* stream);

/* The number of box pixels one workgroup of gpf_accumulate takes: the tests place box areas around its multiples. */
int gpf_pixels_per_workgroup(void);

/* The hot kernel.
 *   vis (N,H,W) u64 as gpr_raster writes it; c (F,3) f64 from gpf_face_normals; poses (N,4,4) f64, object -> camera, row-major,
 *   rows 0..2 are read; K (N,9) f64, row-major, K0 K1 K2 K4 K5 are read; depth (M,H,W) f32, the sensor's z-depth in model units;
 *   frame (N) int32 into M; box (N,4) int32: x0, y0, x1, y1 INCLUSIVE, clamped to the frame by the kernel (x0, y0 up to 0, x1 down
 *   to W-1, y1 down to H-1), a box that is then empty or inverted reads nothing; gate (N), scale (N) f64 (e.g. a multiple of the
 *   diameter, and the diameter)
 *   ->  sums (N,32) int64, 8-byte aligned; status (N) int32.  The call initialises both (to 0).
 * For pair n, with R = rows and columns 0..2 of poses[n], t = its last column, k = K[n], and for every pixel (px, py) of the
 * clamped box whose key is not all ones (covered):
 *     covered += 1
 *     f  = the low 32 bits of the key (unsigned);  zr = (double) the f32 whose bits are the high 32 bits;
 *     dm = (double) depth[frame[n]][py][px];       r = dm - zr
 *     f >= F: status |= GPF_BAD_INDEX, next pixel
 *     m_i = (R_i0*c_f0 + R_i1*c_f1) + R_i2*c_f2   (i = 0, 1, 2);      mm = (m0*m0 + m1*m1) + m2*m2
 *     mm is not below +inf (a NaN included): status |= GPF_BAD_INDEX, next pixel
 *     ASSOCIATED iff dm > 0 and dm < +inf and |r| <= gate[n] and mm > 0; otherwise next pixel
 *     b = ((double)py - k5) / k4;     a = (((double)px - k2) - k1*b) / k0
 *     q = (a*zr, b*zr, zr)            the drawn point;      d = (r*a, r*b, r)     from it to the measured point on the same ray
 *     y_i = (q_i - t_i) / scale[n];   yy = (y0*y0 + y1*y1) + y2*y2
 *     g = (y1*m2 - y2*m1,  y2*m0 - y0*m2,  y0*m1 - y1*m0,  m0, m1, m2)            [y x m, m]
 *     e = ((m0*d0 + m1*d1) + m2*d2) / scale[n];             w = 1.0 / mm
 *     h_i = w*g_i;   term(i,j) = h_i*g_j;   term(i,e) = h_i*e;   term(e,e) = (w*e)*e
 *     the pixel is DROPPED (status |= GPF_RANGE, next pixel) unless yy <= 16 and term(i,i) <= 16 for the six i and
 *     term(e,e) <= 16 (false for a NaN).  Every other |term| is then at most 16 as well (|w g_i g_j| <= the larger square).
 *     count += 1;   every one of the 28 sums += (int64) rint(term * 2^36)          [rint: half to even]
 * Every term is even in m, so the raster's swap of vertices 1 and 2 (a flipped normal) does not matter, and no normal is ever
 * normalised.  With at most 2^22 pixels of |term| <= 16 a sum stays below 2^62.
 * Shape: grid (chunk of gpf_pixels_per_workgroup() box pixels in row-major order of the box, pair); a workgroup whose chunk lies
 * beyond the box returns before it reads a key; one 32-lane atomic add of int64 per workgroup that saw a covered pixel. */
int gpf_accumulate(const unsigned long long* vis, const double* c, int F, const double* poses, const double* K, const float* depth,
                   int M, const int* frame, const int* box, const double* gate, const double* scale, int N, int H, int W,
                   long long* sums, int* status, void* stream);

/* The Gauss-Newton step: one thread per pair.
 *   sums (N,32) from gpf_accumulate; clipped (N) int32 from gpr_raster, or NULL; scale (N) f64; start (N,4,4) f64, or NULL
 *   ->  poses (N,4,4) f64, updated IN PLACE; poses32 (N,4,4) f32, gpr_project's input for the next iteration; state (N) int32,
 *   read and updated (the caller zeroes it before the first iteration).
 * For pair n, in this order:
 *   1. state & GPF_STOP: nothing of the pair is touched.
 *   2. stop = GPF_CLIPPED if clipped and clipped[n] != 0;  else GPF_FEW if count < min_points;  else run 3 to 6, which may
 *      give GPF_DEGENERATE.  A pair that stops now: state |= stop; if start is given, poses[n] = start[n] and poses32[n] = its
 *      f32 conversion (the input pose comes back); else both stay.  GPF_CONVERGED is cleared.  Done.
 *   3. A_ij = (double)sums[ij] * 2^-36 (the conversion of an int64 rounds to nearest even above 2^53, the product is exact);
 *      cnt = (double)count;  A_ii = A_ii + damping*cnt;  rhs_i = (double)sums[21+i] * 2^-36;  thr = min_pivot*cnt.
 *   4. Unpivoted LDL^T, for j = 0..5:
 *         u_k = L_jk*D_k for k < j;    p = A_jj;  p = p - L_jk*u_k for k = 0..j-1 in turn
 *         p is not above thr (a NaN included): GPF_DEGENERATE;    D_j = p
 *         for i = j+1..5:  s = A_ji;  s = s - L_ik*u_k for k = 0..j-1 in turn;  L_ij = s / p
 *   5. z_i = rhs_i;  z_i = z_i - L_ik*z_k for k = 0..i-1 in turn (i = 0..5);   z_i = z_i / D_i;
 *      x_i = z_i;  x_i = x_i - L_ki*x_k for k = i+1..5 in turn (i = 5..0).     xi = x = (omega, tau).
 *   6. xx = ((((x0*x0 + x1*x1) + x2*x2) + x3*x3) + x4*x4) + x5*x5;  xx is not below +inf: GPF_DEGENERATE.
 *   7. The rotation by the Cayley transform of a = 0.5*omega:   s = (a0*a0 + a1*a1) + a2*a2;  p = 1 - s;  q = 1 + s;
 *         Q00 = (p + 2*(a0*a0)) / q     Q01 = (2*(a0*a1) - 2*a2) / q   Q02 = (2*(a0*a2) + 2*a1) / q
 *         Q10 = (2*(a0*a1) + 2*a2) / q   Q11 = (p + 2*(a1*a1)) / q     Q12 = (2*(a1*a2) - 2*a0) / q
 *         Q20 = (2*(a0*a2) - 2*a1) / q   Q21 = (2*(a1*a2) + 2*a0) / q   Q22 = (p + 2*(a2*a2)) / q
 *      = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a): a rotation about omega by 2 atan(|omega| / 2).
 *   8. R'_ij = (Q_i0*R_0j + Q_i1*R_1j) + Q_i2*R_2j;   t'_i = t_i + scale[n]*x_(3+i)   -- the rotation is about the object's
 *      origin (which is why y is taken about t).  Row 3 of the pose is kept.
 *   9. state = (state without GPF_CONVERGED) | (GPF_CONVERGED if xx < tol2).
 *  10. poses[n] = the new pose; poses32[n] = (float) of each of its 16 numbers.
 * min_points >= 0; min_pivot, damping >= 0 and finite; tol2 >= 0 (not a NaN). */
int gpf_update(const long long* sums, const int* clipped, const double* scale, const double* start, int N, long long min_points,
               double min_pivot, double damping, double tol2, double* poses, float* poses32, int* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_REFINE_H */
