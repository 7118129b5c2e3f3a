/*
 * gigapose_coco.h -- C-ABI of libgigapose_coco.so: scoring 2-D detections and segmentations on MI355X (gfx950), the stage behind
 * a detector as gigapose_eval.h is the stage behind the pose estimates.  BOP scores both tasks with COCO's average precision;
 * what that needs on the device is here: the foreground prefix sums of run-length masks (gpc_fg_scan), the intersection of two
 * run-length masks without decoding either (gpc_mask_inter), the same for boxes (gpc_box_inter), COCO's greedy matching of
 * detections to ground truths at several IoU thresholds at once (gpc_match), and the suppression bit matrix of a mask-IoU NMS in
 * the layout gpa_nms_keep reads (gpc_sup_bits).  The AP arithmetic over the matches is the host's
 * (gigapose_amd/detections.py: average_precision).  Nothing of the reference is restated: it installs pycocotools for this; the
 * definitions below ARE the contract.  This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_label.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpc_last_error() returns a thread-local message
 *     for the last failure.  An invalid argument is refused before anything is launched.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/coco_ref.py restates it in numpy and Python integers and must agree bit for
 * bit).  Every decision is taken on integers: no kernel divides and none holds a float, so no result depends on how the work is
 * spread over threads, waves and workgroups or on the order in which they finish.  No atomics.
 *
 * MASKS.  A set of D masks over one H x W frame is (cum int32[total], offsets int32[D+1]) as gpi_rle_scan, gps_rle_string_scan
 * and the gtinfo library's encoder leave them and gpa_run_boxes reads them: mask d owns cum[lo .. hi), lo = offsets[d],
 * hi = offsets[d+1], the inclusive prefix sums of its run lengths over the mask flattened column-major (pixel (y, x) has index
 * x*H + y), the first run being zeros.  Run i (0-based WITHIN the slice) holds the pixel indices [cum[i-1], cum[i]) with
 * cum[-1] = 0 and is foreground iff i is odd.  Mask d is BAD when not (0 <= lo < hi <= total) or cum[hi-1] != HW, HW = H*W (the
 * -1 a failed scan leaves included): gpa_run_boxes' rule.  Every index a kernel forms is bounded by [lo, hi) from `offsets`,
 * never by what cum holds: a fabricated, non-monotone cum may give meaningless numbers but no access outside the arrays.
 */
#ifndef GIGAPOSE_COCO_H
#define GIGAPOSE_COCO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpc_abi_version(void);
const char* gpc_last_error(void);

#define GPC_MAX_ITEMS 65535   /* masks, pairs or groups of one call */
#define GPC_MAX_THRESHOLDS 16
#define GPC_MAX_DEN 65536
#define GPC_MAX_GROUP_GT 4096 /* ground truths of one (image, category) group */
#define GPC_MAX_NMS 2048
#define GPC_MAX_COORD 2097152 /* 2^21: box coordinates are clamped to [-2^21, 2^21] first */

/* status bits of gpc_fg_scan */
#define GPC_BAD_MASK 1 /* the slice is empty or leaves [0, total], or its last prefix sum is not HW */
/* status bits of gpc_mask_inter and gpc_box_inter */
#define GPC_PAIR_RANGE 1 /* pair_a lies outside [0, DA) or pair_b outside [0, DB) */
#define GPC_PAIR_MASK 2  /* the pair touches a BAD mask */
/* status bits of gpc_match */
#define GPC_GROUP_RANGE 1 /* the group's offsets are not ascending or leave the arrays: nothing of the group is written */
#define GPC_GROUP_ORDER 2 /* an ignored ground truth stands before a non-ignored one */
#define GPC_GROUP_SIZE 4  /* more than GPC_MAX_GROUP_GT ground truths */

/* Foreground prefix sums of D masks.
 *   cum, offsets, total, HW as above  ->  fg int32[total], area int64[D] (8-byte aligned), status int32[D].
 * For a mask that is not BAD and i in [lo, hi): fg[i] = the sum over the ODD r <= i - lo of cum[lo + r] - cum[lo + r - 1], the
 * number of foreground pixels in its runs 0 .. i - lo (an int64 sum, stored truncated to 32 bits: it is <= HW < 2^31 for a list
 * a scan wrote); area[d] = that sum at i = hi - 1; status[d] = 0.  A BAD mask: status GPC_BAD_MASK, area 0, its fg NOT written.
 * Shape: one workgroup of 256 threads per mask; chunks of 1024 runs, 4 consecutive runs per thread, the block scan of
 * gp_rle_scan.h (block_inclusive on two alternating LDS slots, one barrier per chunk).
 * Limits: 0 <= D <= 65535 (D = 0 is a no-op after the checks), 0 < HW < 2^31, total >= 0. */
int gpc_fg_scan(const int* cum, const int* offsets, int total, int D, int HW, int* fg, long long* area, int* status, void* stream);

/* Intersections of P pairs of masks: pair p is mask pair_a[p] of set A and mask pair_b[p] of set B (the two sets may be the same
 * arrays), fgA / fgB what gpc_fg_scan wrote for them.
 *   ->  inter int64[P] (8-byte aligned), status int32[P].
 * For a mask M of n = hi - lo runs, with c[j] = cum[lo + j] and f[j] = fg[lo + j], F_M(x) is the number of foreground pixels of
 * M with index < x: with j the FIRST run in [0, n) that has c[j] > x (found by binary search over the slice; j = n if none),
 *     F_M(x) = (j > 0 ? f[j-1] : 0) + (j < n and j odd ? x - c[j-1] : 0).
 * The pair's WALKED mask is the one with fewer runs (A's on a tie), the SEARCHED mask S the other:
 *     inter[p] = the sum over the odd runs i of the walked mask of F_S(c[i]) - F_S(c[i-1])                    (int64)
 * For masks a scan wrote this is the number of pixels set in both, whichever is walked.
 * status: GPC_PAIR_RANGE for an index outside its set, else GPC_PAIR_MASK when either mask is BAD; inter is 0 then, and the
 * other pairs are not affected.
 * Shape: one wave per pair, four pairs per workgroup of 256 threads; lane l takes the odd runs 2l+1, 2l+129, .. of the walked
 * mask (two binary searches each); the 64 partial sums meet in a butterfly of __shfl_xor; lane 0 writes.  Integer addition
 * commutes, so the order of the butterfly does not show.
 * Limits: 0 <= P <= 65535 (P = 0 is a no-op after the checks; the caller chunks), DA, DB >= 0, totalA, totalB >= 0,
 * 0 < HW < 2^31. */
int gpc_mask_inter(const int* cumA, const int* offA, const int* fgA, int totalA, int DA, const int* cumB, const int* offB, const int* fgB,
                   int totalB, int DB, int HW, const int* pair_a, const int* pair_b, int P, long long* inter, int* status, void* stream);

/* Intersections and areas of P pairs of boxes.
 *   boxA (DA, 4), boxB (DB, 4) int32: x0, y0, x1, y1 with x1, y1 EXCLUSIVE
 *   ->  inter, area_a, area_b int64[P] (8-byte aligned), status int32[P].
 * Every coordinate is clamped to [-2^21, 2^21] first.  w = max(0, x1 - x0), h = max(0, y1 - y0), area = w * h; inter = the same
 * of (max x0, max y0, min x1, min y1): the arithmetic of gpa_nms_matrix.  status GPC_PAIR_RANGE and three zeros for an index
 * outside its set.  One thread per pair.  0 <= P <= 65535, DA, DB >= 0. */
int gpc_box_inter(const int* boxA, int DA, const int* boxB, int DB, const int* pair_a, const int* pair_b, int P, long long* inter,
                  long long* area_a, long long* area_b, int* status, void* stream);

/* COCO's matching of detections to ground truths (evaluateImg without crowd regions and without area ranges), at T thresholds.
 *   Q groups, one per (image, category): group q owns the detections [det_off[q], det_off[q+1]) of area_det int64[total_det],
 *   the ground truths [gt_off[q], gt_off[q+1]) of area_gt int64[total_gt] and gt_ignore u8[total_gt], and the row-major block
 *   inter[pair_off[q] + d * G_q + g] of inter int64[total_pair] (d, g counted within the group; D_q x G_q values);
 *   det_off, gt_off int32[Q+1], pair_off int32[Q]; thr_num int32[T]: threshold t is the rational thr_num[t] / thr_den.
 *   The caller supplies a group's detections best first and its ground truths with every non-ignored one before every ignored.
 *   ->  dt_match int32 (T, total_det): the matched ground truth's index WITHIN its group, or -1;
 *       dt_ignore u8 (T, total_det): that ground truth's ignore flag as 0 / 1, 0 when unmatched;  status int32[Q].
 * union(d, g) = area_det[d] + area_gt[g] - inter[d, g].  For threshold t, the group's detections d in order: the candidates are
 * the ground truths g that are not matched at t yet, have union > 0 and
 *     inter * thr_den >= thr_num[t] * union                        (int64, NOT strict: pycocotools skips a g only on <)
 * Of two candidates g, h the better is: the non-ignored one if only one is ignored; else the one of larger IoU, compared as
 * inter_g * union_h against inter_h * union_g in int64; else, the IoUs being equal, the LARGER index (pycocotools' loop
 * replaces its choice on equality, so the last one stands).  d is matched to the best candidate, which is then matched at t;
 * without a candidate dt_match = -1.  This is pycocotools' loop: it walks g in order, stops at the first ignored g once a
 * non-ignored one is held, and otherwise goes on among the ignored ones with the same rule.
 * The caller's duty: 0 <= inter and the areas < 2^31 (masks and boxes of a frame with HW < 2^31); then union < 2^32, and every
 * product stays below 2^63.  Larger values wrap (meaningless matches, no access outside the arrays).
 * status[q]: GPC_GROUP_RANGE when not (0 <= det_off[q] <= det_off[q+1] <= total_det), the same of gt_off, or not
 * (0 <= pair_off[q] and pair_off[q] + D_q * G_q <= total_pair) -- nothing of the group is written but its status; else
 * GPC_GROUP_SIZE when G_q > 4096, GPC_GROUP_ORDER when an ignored ground truth stands before a non-ignored one -- every
 * dt_match of the group is -1 and every dt_ignore 0 then.  D_q = 0 and G_q = 0 are legal.
 * Shape: one wave per (group, threshold), grid (Q, T) of 64 threads.  Lane l holds the ground truths l, l + 64, ..; bit k of a
 * 64-bit register says that l + 64k is matched.  The detections are taken one after the other; each lane keeps its best
 * candidate, a butterfly of __shfl_xor under the total order above gives every lane the wave's.
 * Limits: 0 <= Q <= 65535 (Q = 0 is a no-op after the checks), 1 <= T <= 16, 1 <= thr_den <= 65536 (0 <= thr_num[t] <= thr_den
 * is the caller's duty: the values are on the device), total_det, total_gt, total_pair >= 0. */
int gpc_match(const int* det_off, const int* gt_off, const int* pair_off, int Q, const long long* inter, int total_pair, const long long* area_det,
              int total_det, const long long* area_gt, const unsigned char* gt_ignore, int total_gt, const int* thr_num, int T, int thr_den,
              int* dt_match, unsigned char* dt_ignore, int* status, void* stream);

/* Which mask suppresses which: the bit matrix gpa_nms_matrix writes for boxes, from intersections of any kind.
 *   inter (P, P) int64, of which only the entries [i, j] with i < j are read; area int64[P]; both in suppression order (best
 *   first); the IoU threshold num / den, 0 <= num <= den <= 2^16, den >= 1
 *   ->  sup (P, words) u64, words = (P + 63) / 64, 8-byte aligned; every word is written.
 * union = area[i] + area[j] - inter[i, j].  Bit (j & 63) of sup[i, j / 64] is set iff
 *     j > i  and  j < P  and  inter[i, j] * den > num * union                                                  (int64, STRICT)
 * exactly the layout gpa_nms_keep reads.  The caller's duty: |inter|, |area| < 2^44 (the products stay below 2^62).
 * Shape: one wave per (row, word): lane c tests column 64 * word + c, the 64 answers are one __ballot; four rows per workgroup.
 * 0 <= P <= 2048 (P = 0 is a no-op after the checks). */
int gpc_sup_bits(const long long* inter, const long long* area, int P, int num, int den, unsigned long long* sup, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_COCO_H */
