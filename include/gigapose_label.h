/*
 * gigapose_label.h -- C-ABI of libgigapose_label.so: labelling class-agnostic mask proposals against onboarded objects on MI355X
 * (gfx950), the stage between a segmenter that knows nothing of the objects and the ingest library, whose detections carry a
 * category and a score.  It is what CNOS does between "mask proposals" and "labelled detections": the class token of a DINOv2
 * ViT after the final LayerNorm, L2-normalised, as the descriptor of a crop (gpa_descriptors); its cosine similarity with the
 * descriptors of every template of every object, an object's score the mean of its top k templates, the label the best object
 * (gpa_scores); the tight boxes of masks that arrive without one (gpa_run_boxes); and a greedy box NMS (gpa_nms_matrix,
 * gpa_nms_keep).  Nothing of the reference is restated: it holds no such stage, the definitions below ARE the contract.  This
 * library links no object of the other libraries.
 *
 * Conventions (those of gigapose_maskfit.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpa_last_error() returns a thread-local message
 *     for the last failure.  An invalid argument is refused before anything is launched.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/label_ref.py restates it in numpy and Python integers and must agree bit for
 * bit).  Every DECISION -- which object, which template, which box suppresses which -- is taken on integers, so no result
 * depends on how the work is spread over threads, waves and workgroups or on the order in which they finish.  The one
 * floating-point stage (gpa_descriptors) is IEEE float64 in a summation order fixed below, one rounding per written operation,
 * no fused multiply-add (the library is built with -ffp-contract=off) except inside the correctly rounded square root
 * (gigapose_dist.h states its construction; numpy.sqrt returns the same bits); `/` is the correctly rounded float64 division.
 */
#ifndef GIGAPOSE_LABEL_H
#define GIGAPOSE_LABEL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpa_abi_version(void);
const char* gpa_last_error(void);

/* A descriptor component d in [-1, 1] is stored as rint(d * 2^GPA_Q_BITS) (ties to even), an int32 in [-2^20, 2^20]. */
#define GPA_Q_BITS 20
#define GPA_MAX_C 2048
#define GPA_MAX_K 64
#define GPA_MAX_BANK 1048576 /* O * T of one gpa_scores call */
#define GPA_MAX_NMS 8192
#define GPA_MAX_COORD 2097152 /* 2^21: box coordinates are clamped to [-2^21, 2^21] before the NMS arithmetic */

/* status bits of gpa_descriptors */
#define GPA_NON_FINITE 1 /* a value of the crop's class token is NaN or infinite, or the squared norm is */
#define GPA_ZERO_NORM 2  /* the normalised token is all zeros (a constant token with beta = 0) */
/* status bits of gpa_run_boxes */
#define GPA_EMPTY_MASK 1 /* the mask has no set pixel */
#define GPA_BAD_MASK 2   /* the slice of the detection is empty or leaves [0, total], or its last prefix sum is not H*W */

/* The descriptors of B crops.
 *   x f32: value c of crop b's class token is x[b * crop_stride + c * channel_stride] (strides in ELEMENTS, both > 0): the
 *   contiguous (B, 257, C) tensor has strides (257 * C, 1), the ViT workspace's channel-major view (C, mpad) has (257, mpad).
 *   Nothing but these B * C values is read.  gamma, beta f32 (C): the final LayerNorm's weight and bias; eps its epsilon.
 *   ->  q (B, C) int32, status (B) int32.  B >= 0 (B = 0 is a no-op after the checks), C a multiple of 64, 64 <= C <= 2048.
 * One workgroup of 256 threads per crop.  SUM(v): thread t adds v[c] for c = t, t + 256, t + 512, .. < C in that order to a
 * partial that starts at +0.0 (threads with t >= C keep +0.0); then for off = 128, 64, .. 1: partial[t] += partial[t + off]
 * for t < off; the sum is partial[0].  With every f32 widened to float64 first:
 *     mean = SUM(x) / C;   dev[c] = x[c] - mean;   var = SUM(dev * dev) / C;   r = 1 / root(var + eps)
 *     y[c] = (dev[c] * r) * gamma[c] + beta[c];     n2 = SUM(y * y);   norm = root(n2)
 *     q[b, c] = (int) rint((y[c] / norm) * 2^20)
 * status[b] = GPA_NON_FINITE when an x[c] is not finite or n2 is not finite; else GPA_ZERO_NORM when n2 == 0; else 0.  A
 * flagged row of q is all zeros. */
int gpa_descriptors(const float* x, long long crop_stride, long long channel_stride, const float* gamma, const float* beta, double eps,
                    int B, int C, int* q, int* status, void* stream);

/* Labels and scores of P proposals against a bank of O objects x T templates.
 *   q (P, C) int32, bank (O, T, C) int32, every value in [-2^20, 2^20] (the caller's duty: with larger values the int64 sums
 *   wrap); k: the number of templates an object's score is taken over.
 *   ->  dot (P, O, T) int64, 8-byte aligned: dot[p, o, t] = sum over c of q[p, c] * bank[o, t, c], exact (|dot| <= C * 2^40 <
 *       2^52);
 *       obj (P, O) int64 or NULL: the sum of the kk = min(k, T) largest values of dot[p, o, :] -- a multiset sum, so it does
 *       not matter which of several equal dots is taken;
 *       label (P) int32: the FIRST o that attains the largest obj[p, :];   score (P) int64, 8-byte aligned: that sum (the
 *       float score is score / (kk * 2^40));   best_template (P) int32: the FIRST t that attains the largest dot[p, label, :].
 * P >= 0 (P = 0 is a no-op after the checks), O, T >= 1, O * T <= 2^20, 1 <= C <= 2048, 1 <= k <= 64, P * O * T < 2^40.
 * Shape: dots_kernel, grid (64 bank rows, 64 proposals), tiles q and the bank through LDS 32 channels at a time, a thread
 * holds 4 x 4 int64 sums; select_kernel, one workgroup per proposal, a wave per object: kk passes, each taking the largest
 * (value, then smallest t) below the one taken before. */
int gpa_scores(const int* q, const int* bank, int P, int O, int T, int C, int k, long long* dot, long long* obj, int* label,
               long long* score, int* best_template, void* stream);

/* Tight boxes and areas of D run-length masks, in closed form from the runs.
 *   cum int32[total], offsets int32[D+1]: as gpi_rle_scan (or gps_rle_string_scan) leaves them and gpm_mask_moments takes them:
 *   detection d owns cum[lo .. hi), lo = offsets[d], hi = offsets[d+1], the inclusive prefix sums of its run lengths over the
 *   H x W mask flattened column-major (pixel (y, x) has index x*H + y)
 *   ->  box (D, 4) int32: x0, y0, x1, y1 with x1, y1 EXCLUSIVE;  area (D) int64, 8-byte aligned;  status (D) int32.
 * Detection d is BAD when not (0 <= lo < hi <= total) or cum[hi-1] != H*W (a -1 included): status GPA_BAD_MASK, box and area 0.
 * Else, for every i = lo+1, lo+3, .. < hi (the runs of ones), with a = cum[i-1], b = cum[i]: the run holds the pixel indices
 * [a, b); a run with not (0 <= a < b <= H*W) adds nothing.  With xa = a / H, ya = a % H, xb = (b-1) / H, yb = (b-1) % H:
 *     area += b - a;   x0 = min(x0, xa);   x1 = max(x1, xb + 1)
 *     xa == xb:  y0 = min(y0, ya);  y1 = max(y1, yb + 1)         (a column segment)
 *     else:      y0 = 0;  y1 = H                                  (the run reaches the bottom of column xa and the top of xb)
 * area == 0: status GPA_EMPTY_MASK and the box 0, 0, 0, 0.  No pixel is visited.
 * Limits: 0 <= D <= 65535 (D = 0 is a no-op after the checks), H, W > 0, H*W < 2^31, total >= 0. */
int gpa_run_boxes(const int* cum, const int* offsets, int total, int D, int H, int W, int* box, long long* area, int* status, void* stream);

/* Which box suppresses which.
 *   box (P, 4) int32 x0, y0, x1, y1 (exclusive), label (P) int32 (read only if per_label != 0), both ALREADY in suppression
 *   order (best first); 0 <= num <= den <= 2^16, den >= 1: the IoU threshold num / den
 *   ->  sup (P, words) u64, words = (P + 63) / 64, 8-byte aligned; every word is written.
 * Every coordinate is clamped to [-2^21, 2^21] first.  w = max(0, x1 - x0), h = max(0, y1 - y0), area = w * h; inter = the
 * same of (max x0, max y0, min x1, min y1); union = area_i + area_j - inter.  Bit (j & 63) of sup[i, j / 64] is set iff
 *     j > i  and  j < P  and  (per_label == 0 or label[i] == label[j])  and  inter * den > num * union        (int64, STRICT)
 * No division is taken; both products stay below 2^62.  0 <= P <= 8192 (P = 0 is a no-op after the checks). */
int gpa_nms_matrix(const int* box, const int* label, int P, int num, int den, int per_label, unsigned long long* sup, void* stream);

/* The greedy pass.  sup as above -> keep (P) u8: keep[i] = 1 iff no j < i with keep[j] = 1 has bit i set in its row; else 0.
 * One workgroup; a box that is itself suppressed suppresses nothing.  0 <= P <= 8192. */
int gpa_nms_keep(const unsigned long long* sup, int P, unsigned char* keep, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_LABEL_H */
