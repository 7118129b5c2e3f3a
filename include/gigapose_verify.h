/*
 * gigapose_verify.h -- C-ABI of libgigapose_verify.so: verifying pose hypotheses against the sensor's depth image and the
 * detection's mask on MI355X (gfx950), the stage that chooses among the k hypotheses of one detection.  A hypothesis is drawn
 * by libgigapose_render.so (gpr_project + gpr_raster: a z-buffer of 64-bit keys); every pixel of its box is then classified by
 * how the measured depth compares with the drawn one (agrees, lies behind the drawn surface, lies in front of it, is not
 * measured) and by whether the detection's run-length mask (as libgigapose_ingest.so's gpi_rle_scan leaves it) holds the pixel,
 * and the classes are COUNTED (gpv_counts, the hot kernel).  What is made of the counts -- a depth fit, an intersection over
 * union, their product -- is host arithmetic (gigapose_amd/verify.py: verification_scores).  Reference: the role of the
 * multi-hypothesis refiners (n_pose_hypotheses: 5 in src/megapose/utils/load_model.py:27-45, refiner_utils.py:35: refine all,
 * keep the one that fits the image best); nothing of them is restated, the definitions below ARE the contract.  This library
 * links no object of the other libraries.
 *
 * Conventions (those of gigapose_refine.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpv_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Limits: N <= 65535 per call (the grid's second dimension; gigapose_amd/verify.py chunks the pairs), 1 <= H*W <= 2^22,
 * M >= 1 where depth is given, D >= 0 and total >= 0 where masks are given; every buffer is addressed through size_t (the key
 * buffer passes 2^31 elements at 874 pairs of 480 x 640).  N = 0 is a no-op that returns 0 after the sizes have been checked.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/verify_ref.py restates it in numpy and must agree bit for bit).  All
 * floating-point work is IEEE float64, one rounding per written operation, no fused multiply-add (the library is built with
 * -ffp-contract=off); `/` is the correctly rounded float64 division.  Only INTEGERS are summed, so no result depends on how
 * the pixels are spread over threads, waves and workgroups, or on the order in which they finish.
 */
#ifndef GIGAPOSE_VERIFY_H
#define GIGAPOSE_VERIFY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpv_abi_version(void);
const char* gpv_last_error(void);

/* Layout of one pair's row of counts: 16 int64 = 128 bytes.
 *   [2*class + in_mask] for the four classes of a COVERED pixel: 0 1 unmeasured, 2 3 agree, 4 5 behind, 6 7 front
 *   8   pixels of the box that the mask holds and the drawing does not cover
 *   9   the sum over the AGREE pixels of rint(q * 2^20), q = |r| / tol in [0, 1]
 *   10 .. 15  always 0 */
#define GPV_COUNTS 16
#define GPV_UNMEASURED 0 /* no depth image, or the measurement is not in (0, +inf), or r or tol is a NaN */
#define GPV_AGREE 1      /* |r| <= tol */
#define GPV_BEHIND 2     /* r > tol: the sensor sees through the drawn surface, a free-space violation */
#define GPV_FRONT 3      /* r < -tol: something lies in front of the drawn surface, an occluder or a contradiction */
#define GPV_UNCOVERED_IN_MASK 8
#define GPV_RESIDUAL 9
#define GPV_QUANTUM_BITS 20 /* q is added as rint(q * 2^20) */

/* status */
#define GPV_BAD_FRAME 1 /* depth is given and frame[n] lies outside [0, M) */
#define GPV_BAD_MASK 2  /* det[n] >= D, or the slice of det[n] is empty or leaves [0, total], or its last prefix sum is not H*W */

/* The number of box pixels one workgroup of gpv_counts takes: the tests place box areas around its multiples. */
int gpv_pixels_per_workgroup(void);

/* The hot kernel.
 *   vis (N,H,W) u64 as gpr_raster writes it, 8-byte aligned;
 *   depth (M,H,W) f32, the sensor's z-depth in model units, or NULL: no depth image; frame (N) int32 into M, read only where
 *   depth is given (and then required);
 *   cum int32[total], offsets int32[D+1]: the run-length masks of D detections as gpi_rle_scan (or gps_rle_string_scan) leaves
 *   them -- detection d owns cum[offsets[d] .. offsets[d+1]), the inclusive prefix sums of its run lengths over the mask
 *   flattened COLUMN-major (gigapose_ingest.h: pixel (x, y) has index p = x*H + y, the first run is zeros), a bad list has -1
 *   as its last entry -- or cum NULL: no masks, and then offsets and det are not read;
 *   det (N) int32 into D, -1 (any negative value) = this pair has no mask; several pairs may name one detection (the k
 *   hypotheses of a detection share its mask); NULL is allowed if and only if cum is NULL;
 *   box (N,4) int32: x0, y0, x1, y1 INCLUSIVE, clamped to the frame by the kernel (x0, y0 up to 0, x1 down to W-1, y1 down to
 *   H-1), a box that is then empty or inverted reads nothing; tol (N) f64 (e.g. a multiple of the diameter)
 *   ->  counts (N,16) int64, 8-byte aligned; status (N) int32.  The call initialises both (to 0).
 * Pair rules, checked for EVERY pair (whatever its box) before a key, a depth or a prefix sum other than the slice's last is
 * read; a pair that breaks one sets the bit, reads nothing more and leaves its row 0:
 *     depth is given and frame[n] is not in [0, M):                                  status |= GPV_BAD_FRAME
 *     cum is given and det[n] >= 0 and one of: det[n] >= D;  with lo = offsets[det[n]], hi = offsets[det[n] + 1] not
 *     (0 <= lo < hi <= total) [list_range of gp_rle_scan.h];  cum[hi - 1] != H*W:    status |= GPV_BAD_MASK
 * (both bits where both rules are broken).  For every other pair and every pixel (px, py) of its clamped box:
 *     covered = the key is not all ones
 *     in_mask = 0 when cum is NULL or det[n] < 0; else with p = px*H + py:  #{i in [lo, hi) : cum[i] <= p} & 1
 *     not covered:  counts[8] += in_mask;  next pixel
 *     zr = (double) the f32 whose bits are the high 32 bits of the key
 *     class = GPV_UNMEASURED when depth is NULL; else with dm = (double) depth[frame[n]][py][px]:
 *         GPV_UNMEASURED unless dm > 0 and dm < +inf; else with r = dm - zr, t = tol[n], in this order
 *         |r| <= t: GPV_AGREE;   else r > t: GPV_BEHIND;   else r < -t: GPV_FRONT;   else GPV_UNMEASURED (r or t is a NaN)
 *     counts[2*class + in_mask] += 1
 *     GPV_AGREE:  q = t > 0 ? |r| / t : 0;   counts[9] += (int64) rint(q * 2^20)          [rint: half to even]
 *                 (a q that is a NaN -- |r| = t = +inf, which takes a key whose depth is -inf -- adds 0)
 * With at most 2^22 pixels of q <= 1 a sum stays below 2^43.
 * Shape: grid (chunk of gpv_pixels_per_workgroup() box pixels in row-major order of the box, pair); a workgroup whose chunk
 * lies beyond the box returns before it reads a key; a thread keeps its ten counters in registers; wave shuffles, LDS, then
 * one atomic add of int64 per counter that is not 0, by the workgroups that saw a covered or a masked pixel. */
int gpv_counts(const unsigned long long* vis, const float* depth, int M, const int* frame, const int* cum, const int* offsets,
               int total, int D, const int* det, const int* box, const double* tol, int N, int H, int W, long long* counts,
               int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_VERIFY_H */
