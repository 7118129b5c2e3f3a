/*
 * gigapose_maskfit.h -- C-ABI of libgigapose_maskfit.so: fitting coarse poses to the detection's mask on MI355X (gfx950), the
 * stage between the coarse pose and the depth refiner (or, on an RGB-only run, the only refinement there is).  The four degrees
 * of freedom the coarse stage regresses per correspondence -- the in-plane angle, the scale (so t_z) and the 2-D translation --
 * are exactly what a silhouette's moments of order 0, 1 and 2 hold: the pose is drawn by libgigapose_render.so (gpr_project +
 * gpr_raster: a z-buffer of 64-bit keys), the moments of its covered pixels are summed over its box together with its
 * intersection with the detection's run-length mask (gpm_moments, the hot kernel), the moments of the mask itself are summed in
 * closed form from its runs (gpm_mask_moments, once per detection), and a rational rule moves the pose so that the drawing's
 * moments meet the mask's, keeping the pose of the best intersection over union seen so far (gpm_update).  Nothing of the
 * reference is restated: it has no such stage, the definitions below ARE the contract.  This library links no object of the
 * other libraries.
 *
 * Conventions (those of gigapose_verify.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpm_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Limits: N <= 65535 per call (the grid's second dimension; gigapose_amd/maskfit.py chunks the pairs), 1 <= H*W <= 2^22,
 * H <= 16384 and W <= 16384 (a sum of x*x over 2^22 pixels then stays below 2^50: every sum is exact as an int64 AND as a
 * double), D >= 0, total >= 0; every buffer is addressed through size_t (the key buffer passes 2^31 elements at 874 pairs of
 * 480 x 640).  N = 0 (D = 0 for gpm_mask_moments) is a no-op that returns 0 after the sizes have been checked.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/maskfit_ref.py restates it and must agree bit for bit).  Only INTEGERS are
 * summed, so no result depends on how pixels or runs are spread over threads, waves and workgroups, or on the order in which
 * they finish.  All floating-point work (gpm_update only) is IEEE float64, one rounding per written operation, in the written
 * order, no fused multiply-add (the library is built with -ffp-contract=off); `/` is the correctly rounded float64 division.
 * There is no square root and no transcendental function anywhere on the device: the turn is the rational parametrisation of
 * the circle by tan(angle / 2), the scale is one step of Heron's iteration.
 */
#ifndef GIGAPOSE_MASKFIT_H
#define GIGAPOSE_MASKFIT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpm_abi_version(void);
const char* gpm_last_error(void);

/* Layout of a row of moments.  A mask's row (gpm_mask_moments) has 8 int64, a pair's row (gpm_moments) 16 = 128 bytes:
 *   0 n   1 sum x   2 sum y   3 sum x*x   4 sum x*y   5 sum y*y     over the set's pixels (x, y), x the column
 *   6   pair: the covered pixels that the mask holds (the intersection);  mask: 0
 *   7   pair: the covered pixels on an edge of the clamped box that is not an edge of the frame;  mask: 0
 *   8 .. 15  always 0 */
#define GPM_MASK_ROW 8
#define GPM_ROW 16
#define GPM_INTER 6
#define GPM_EDGE 7

/* status bits.  The first two are set by gpm_mask_moments (BAD_MASK) and gpm_moments, the others by gpm_update; the first
 * four are the STOP bits. */
#define GPM_BAD_MASK 1      /* det[n] >= D, or the slice of the detection is empty or leaves [0, total], or its last prefix sum is not H*W */
#define GPM_NO_MASK 2       /* det[n] < 0 */
#define GPM_FEW 4           /* the drawing or the mask has fewer pixels than min_points */
#define GPM_CLIPPED 8       /* the view dropped a triangle (clipped[n] != 0) */
#define GPM_ROUND 16        /* the last step took no turn: a set is too round, or the two orientations are more than 45 degrees apart */
#define GPM_NOT_IMPROVED 32 /* the best pose is the input pose */
#define GPM_STOP (GPM_BAD_MASK | GPM_NO_MASK | GPM_FEW | GPM_CLIPPED)

/* The moments of every detection's mask, in closed form from its runs.
 *   cum int32[total], offsets int32[D+1]: the run-length masks of D detections as gpi_rle_scan (or gps_rle_string_scan) leaves
 *   them -- detection d owns cum[lo .. hi), lo = offsets[d], hi = offsets[d+1], the inclusive prefix sums of its run lengths
 *   over the mask flattened COLUMN-major (pixel (x, y) has index p = x*H + y, the first run is zeros), a bad list has -1 as its
 *   last entry
 *   ->  mm (D,8) int64, 8-byte aligned; mstatus (D) int32.  Every entry of both is written.
 * Detection d is BAD when not (0 <= lo < hi <= total) [list_range of gp_rle_scan.h] or cum[hi-1] != H*W (a -1 included):
 * mstatus[d] = GPM_BAD_MASK and its row is 0.  Else mstatus[d] = 0 and, for every i = lo+1, lo+3, .. < hi (the runs of ones),
 * with a = cum[i-1], b = cum[i]: the run holds the pixel indices [a, b); a run with not (0 <= a < b <= H*W) adds nothing
 * (zero-length runs).  With xa = a / H, ya = a % H, xb = (b-1) / H, yb = (b-1) % H, S1(m) = m(m+1)/2, S2(m) = m(m+1)(2m+1)/6:
 *   a column segment (x, y0 .. y1):  n = y1-y0+1;  sy = S1(y1) - S1(y0-1);  syy = S2(y1) - S2(y0-1);
 *                                    adds  n,  x*n,  sy,  x*x*n,  x*sy,  syy
 *   full columns x0 .. x1:           c = x1-x0+1;  sx = S1(x1) - S1(x0-1);  sxx = S2(x1) - S2(x0-1);
 *                                    adds  c*H,  H*sx,  c*S1(H-1),  H*sxx,  sx*S1(H-1),  c*S2(H-1)
 *   xa == xb: the segment (xa, ya .. yb);   else the segments (xa, ya .. H-1) and (xb, 0 .. yb), and, when xb - xa >= 2, the
 *   full columns xa+1 .. xb-1.
 * No pixel is visited.  Every product stays below 2^63 under the limits (S2(16383) * 16384 < 2^57).
 * Shape: one workgroup per detection, its runs strided over the threads; wave shuffles, LDS, plain vector stores. */
int gpm_mask_moments(const int* cum, const int* offsets, int total, int D, int H, int W, long long* mm, int* mstatus, void* stream);

/* The number of box pixels one workgroup of gpm_moments takes: the tests place box areas around its multiples. */
int gpm_pixels_per_workgroup(void);

/* The hot kernel.
 *   vis (N,H,W) u64 as gpr_raster writes it, 8-byte aligned; cum, offsets, total, D as above; det (N) int32 into D (several
 *   pairs may name one detection); box (N,4) int32: x0, y0, x1, y1 INCLUSIVE, clamped to the frame by the kernel (x0, y0 up to
 *   0, x1 down to W-1, y1 down to H-1), a box that is then empty or inverted reads nothing
 *   ->  rows (N,16) int64, 8-byte aligned; status (N) int32.  The call initialises both (to 0).
 * Pair rules, checked for EVERY pair (whatever its box) before a key or a prefix sum other than the slice's last is read; a
 * pair that breaks one sets the bit, reads nothing more and leaves its row 0:
 *     det[n] < 0:                                                                              status |= GPM_NO_MASK
 *     det[n] >= D;  or not (0 <= lo < hi <= total);  or cum[hi - 1] != H*W  (gpv_counts' rules):  status |= GPM_BAD_MASK
 * For every other pair and every pixel (px, py) of its clamped box (X0, Y0, X1, Y1) whose key is not all ones (COVERED):
 *     rows[0..5] += 1, px, py, px*px, px*py, py*py
 *     rows[6]    += #{i in [lo, hi) : cum[i] <= p} & 1,  p = px*H + py         (the bisection is run for covered pixels only)
 *     rows[7]    += 1 when (px == X0 and X0 > 0) or (px == X1 and X1 < W-1) or (py == Y0 and Y0 > 0) or (py == Y1 and Y1 < H-1)
 * A row whose slot 7 is not 0 belongs to a drawing that may go on beyond its box: its moments are those of a part.
 * Shape: grid (chunk of gpm_pixels_per_workgroup() box pixels in row-major order of the box, pair); a workgroup whose chunk
 * lies beyond the box returns before it reads a key; a thread keeps its eight counters in registers; wave shuffles, LDS, then
 * one atomic add of int64 per counter that is not 0. */
int gpm_moments(const unsigned long long* vis, const int* cum, const int* offsets, int total, int D, const int* det, const int* box,
                int N, int H, int W, long long* rows, int* status, void* stream);

/* The step: one thread per pair.
 *   rows (N,16), status (N) from gpm_moments at the CURRENT pose; mm (D,8) from gpm_mask_moments; det (N); clipped (N) int32
 *   from gpr_raster, or NULL; K (N,9) f64, row-major 3 x 3; start (N,4,4) f64: the input poses; it >= 0: the number of this
 *   call in the loop; last != 0: judge only
 *   ->  IN PLACE: poses (N,4,4) f64; poses32 (N,4,4) f32, gpr_project's input for the next iteration; best (N,4,4) f64, the best
 *   pose so far; score (N,4) int64: intersection and union of the best pose, intersection and union of the input pose; state
 *   (N,2) int32: the status bits, the iteration the best pose came from.  The call with it == 0 initialises best, score and
 *   state; the caller need not.
 * For pair n, in this order:
 *   0. it == 0:  best = poses[n];  score = (0, 1, 0, 1);  state = (0, 0).
 *   1. state[0] & GPM_STOP: nothing more of the pair is touched.
 *   2. stop = status[n] & (GPM_BAD_MASK | GPM_NO_MASK);  when that is 0 and det[n] is not in [0, D): GPM_NO_MASK for a
 *      negative det[n], else GPM_BAD_MASK;  |= GPM_CLIPPED when clipped and clipped[n] != 0;  when still 0, with D_ = rows[n]
 *      and M_ = mm[det[n]]:  GPM_FEW when D_0 < min_points or M_0 < min_points.
 *      A pair that stops: state[0] = (state[0] without GPM_ROUND) | stop | GPM_NOT_IMPROVED;  state[1] = 0;  poses[n] = best =
 *      start[n];  poses32[n] = its f32 conversion;  score[0], score[1] = score[2], score[3].  Done: the input pose comes back,
 *      for good, with what is known of it.
 *   3. inter = D_6;  uni = D_0 + M_0 - inter  (int64).
 *      it == 0:  score = (inter, uni, inter, uni)   [the input pose is the first best, whatever its slot 7].
 *      else, when D_7 == 0 and inter * score[1] > score[0] * uni  (int64, exact: an equal ratio keeps the earlier pose):
 *          best = poses[n];  score[0], score[1] = inter, uni;  state[1] = it.
 *   4. last:  poses[n] = best;  poses32[n] = its f32 conversion;  state[0] |= GPM_NOT_IMPROVED when state[1] == 0.  Done.
 *   5. Shape values of both sets S in (D_, M_), n = (double)S_0 (conversions of integers below 2^53 are exact):
 *          mx = S_1/n;  my = S_2/n;  uxx = S_3/n - mx*mx;  uxy = S_4/n - mx*my;  uyy = S_5/n - my*my
 *          a = uxx - uyy;  b = 2*uxy;  tr = uxx + uyy
 *   6. The turn.  e2 = min_elongation*min_elongation;  dot = aD*aM + bD*bM;  cross = aD*bM - bD*aM;
 *      turned = aD*aD + bD*bD >= e2*(trD*trD)  and  aM*aM + bM*bM >= e2*(trM*trM)  and  dot > 0  and  |cross| <= dot
 *      (false where a NaN takes part);   tau = turned ? (gain*(cross/dot)) / 4 : 0;
 *      tt = tau*tau;  den = 1 + tt;  c = (1 - tt)/den;  s = (2*tau)/den        -- the turn by 2 atan(tau) about the camera's z
 *      axis; cross/dot is the tangent of TWICE the angle between the two sets' principal axes.
 *      P = poses[n];  for j = 0..3:  Q_0j = c*P_0j - s*P_1j;   Q_1j = s*P_0j + c*P_1j;   rows 2 and 3 are kept.
 *   7. The scale.  g = (1 + (double)D_0/(double)M_0) / 2;   g = 1 + gain*(g - 1);   g < 0.5: g = 0.5;  g > 2: g = 2
 *      -- with u = t_z / its true value, D_0/M_0 = 1/u^2 and g*u = (u + 1/u)/2, Heron's step towards 1.
 *   8. The shift.  With k = K[n] and t = (Q_03, Q_13, Q_23):
 *          ox = ((k0*t0 + k1*t1) + k2*t2) / t2;   oy = ((k3*t0 + k4*t1) + k5*t2) / t2      the origin's projection after the turn
 *          dx = mxD - k2;  dy = myD - k5;   px = k2 + (c*dx - s*dy);   py = k5 + (s*dx + c*dy)   the drawn centroid, turned
 *          qx = ox + (px - ox)/g;   qy = oy + (py - oy)/g                                 ... and scaled about the origin
 *          t0 = g*t0;  t1 = g*t1;  t2 = g*t2
 *          Q_03 = t0 + ((gain*(mxM - qx))*t2)/k0;   Q_13 = t1 + ((gain*(myM - qy))*t2)/k4;   Q_23 = t2
 *   9. poses[n] = Q;  poses32[n] = (float) of each of its 16 numbers;  state[0] = (state[0] without GPM_ROUND) | (GPM_ROUND
 *      unless turned).
 * min_points >= 1; min_elongation and gain finite, min_elongation >= 0, 0 < gain <= 1. */
int gpm_update(const long long* rows, const int* status, const long long* mm, int D, const int* det, const int* clipped, const double* K,
               const double* start, int N, int it, int last, long long min_points, double min_elongation, double gain, double* poses,
               float* poses32, double* best, long long* score, int* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_MASKFIT_H */
