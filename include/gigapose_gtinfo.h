/*
 * gigapose_gtinfo.h -- C-ABI of libgigapose_gtinfo.so: what a BOP dataset's scene_gt_info.json and mask / mask_visib images
 * hold, computed on MI355X (gfx950) for ground truths drawn by libgigapose_render.so: px_count_all / px_count_valid /
 * px_count_visib (and with them visib_fract), bbox_obj / bbox_visib, and the two masks as uncompressed COCO run lengths.
 * bop_toolkit produces these with an OpenGL renderer (scripts/calc_gt_info.py, calc_gt_masks.py); an Instinct accelerator has
 * none.  A ground truth is drawn by gpr_project + gpr_raster (a z-buffer of 64-bit keys) on a CANVAS that contains the frame;
 * gpg_classify judges every pixel against the sensor's depth by the BOP-19 visibility rule, word for word as
 * gigapose_eval.h states it on ray distances; gpg_count_runs + gpg_write_runs are the run-length ENCODER, the inverse of
 * what gpi_rle_scan and gps_rle_string_scan decode.  The definitions below ARE the contract: bop_toolkit is not consulted.
 * This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_verify.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpg_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Limits, refused with -1 and a message before anything is launched: N <= 65535 per call (the grid's second dimension;
 * gigapose_amd/gtinfo.py chunks the instances), the frame has 1 <= H*W <= 2^22, the canvas Hc*Wc < 2^31 with Hc, Wc <= 2^30
 * (a frame coordinate then stays inside the boxes' initial values), 0 <= ox, ox + W <= Wc, 0 <= oy, oy + H <= Hc, M >= 1
 * where depth is given, R >= 1, delta not a NaN, which 0 or 1, total >= 0.  Every buffer is addressed through size_t (the
 * keys pass 2^31 bytes at 98 instances of a 1440 x 1920 canvas).  N = 0 is a no-op that returns 0 after the sizes have been
 * checked.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/gtinfo_ref.py restates it in numpy and must agree bit for bit).  The one
 * floating-point step is (Dm - Dt) <= delta in IEEE float64, one rounding per written operation, no fused multiply-add (the
 * library is built with -ffp-contract=off).  Only INTEGERS are merged (sums, minima, maxima), so no result depends on how
 * the pixels are spread over threads, waves and workgroups, or on the order in which they finish.
 */
#ifndef GIGAPOSE_GTINFO_H
#define GIGAPOSE_GTINFO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpg_abi_version(void);
const char* gpg_last_error(void);

/* a row of info: 4 int64 */
#define GPG_INFO 4
#define GPG_PX_ALL 0      /* object pixels of the WHOLE canvas: px_count_all */
#define GPG_PX_FRAME 1    /* object pixels inside the frame */
#define GPG_PX_VALID 2    /* object pixels inside the frame where the sensor measured (dt > 0): px_count_valid */
#define GPG_PX_VISIB 3    /* visible pixels: px_count_visib */
/* a row of box: 8 int32 = min x, min y, max x, max y of the object pixels of the canvas, then of the visible pixels, in FRAME
 * coordinates (the first four may be negative or >= W, H); a set that is empty keeps the initial values */
#define GPG_BOX 8
#define GPG_BOX_EMPTY_MIN 1073741824    /*  2^30 */
#define GPG_BOX_EMPTY_MAX -1073741824   /* -2^30 */
/* a byte of cls */
#define GPG_CLS_OBJECT 1
#define GPG_CLS_VISIBLE 2
/* status */
#define GPG_BAD_FRAME 1 /* depth is given and frame[n] lies outside [0, M) */
#define GPG_BAD_RAY 2   /* ray_index[n] lies outside [0, R) */

/* The canvas.  The keys are drawn on (N,Hc,Wc); frame pixel (x, y) is canvas pixel (x + ox, y + oy): a ground truth that
 * leaves the frame loses the part outside from its visible fraction, and its amodal box extends beyond the frame.
 * Hc = H, Wc = W, ox = oy = 0 is allowed.
 *   vis (N,Hc,Wc) u64 as gpr_raster writes it, 8-byte aligned;
 *   depth (M,H,W) f32, the sensor's z-depth in model units, or NULL: no depth image; frame (N) int32 into M, read only where
 *   depth is given (and then required);
 *   ray (R,H,W) f64, ray_index (N) int32 into R: exactly gpe_vsd_counts' ray map (gigapose_eval.h), over the FRAME;  delta f64
 *   ->  cls (N,W,H) u8, COLUMN-major: the byte of frame pixel (x, y) of instance n sits at n*W*H + x*H + y, the order in which
 *       gigapose_ingest.h flattens masks; bit 0 = object, bit 1 = visible;
 *       info (N,4) int64, 8-byte aligned;  box (N,8) int32;  status (N) int32.
 * The call initialises all four outputs (cls, info, status to 0; a row of box to 2^30, 2^30, -2^30, -2^30 twice).
 * Pair rules, checked before any key is read; a pair that breaks one sets its bit, reads nothing and leaves its rows at their
 * initial values with cls all 0:
 *     depth is given and frame[n] is not in [0, M):   status |= GPG_BAD_FRAME
 *     ray_index[n] is not in [0, R):                  status |= GPG_BAD_RAY
 * Per canvas pixel:
 *     dm = the f32 whose bits are the key's high word
 *     object = the key is not all ones and 0 < dm < +inf
 * Per frame pixel:
 *     dt = the sensor's depth there; a value that is negative, NaN or infinite counts as 0, and so does every pixel when depth
 *          is NULL
 *     Dm = (double)dm * ray      Dt = (double)dt * ray                                        [one rounding each]
 *     visible = object && ((dt > 0 && (Dm - Dt) <= delta) || dt == 0)                          [the BOP-19 visibility]
 * info[0] counts the object pixels of the whole canvas, info[1] those inside the frame, info[2] those inside the frame with
 * dt > 0, info[3] the visible pixels.  box[0..3] is taken over the object pixels of the canvas, box[4..7] over the visible
 * pixels, merged with 32-bit integer atomic min / max.
 * Shape: grid (64 x 64 canvas tile, instance); a wave's 8-byte key loads are contiguous within a row; the class bytes of a
 * tile are transposed through LDS so that the column-major stores are contiguous too; a tile wholly outside the frame only
 * counts; counters and box corners are reduced by wave shuffles, then LDS, then one atomic per value that is not neutral. */
int gpg_classify(const unsigned long long* vis, int Hc, int Wc, int ox, int oy, const float* depth, int M, const int* frame,
                 const double* ray, int R, const int* ray_index, double delta, int N, int H, int W, unsigned char* cls,
                 long long* info, int* box, int* status, void* stream);

/* The chunk C of column-major pixels a workgroup of the two run kernels takes: the tests place edges around its multiples. */
int gpg_pixels_per_workgroup(void);

/* Bytes of the workspace of the two run kernels: per (instance, chunk) two int32, the chunk's number of transitions and the
 * position of its last one.  0 if an argument is out of range. */
size_t gpg_runs_workspace_bytes(int N, int H, int W);

/* The length of each instance's run list.  cls (N,W,H) u8 as gpg_classify writes it; which = 0: the object bit, 1: the visible
 * bit  ->  runs (N) int32; workspace: gpg_runs_workspace_bytes(N, H, W) bytes, 8-byte aligned.  The call initialises both.
 * With v(p) the chosen bit of column-major pixel p = x*H + y and v(-1) = 0, the transitions are the p in [0, H*W) with
 * v(p) != v(p-1), and runs[n] = their number + 1: the length of COCO's uncompressed `counts`, whose first run is zeros (of
 * length 0 when pixel 0 is set). */
int gpg_count_runs(const unsigned char* cls, int N, int H, int W, int which, int* runs, void* workspace, void* stream);

/* The lists.  The same cls, which and workspace (as gpg_count_runs left it); offsets (N+1) int32: instance n owns
 * [offsets[n], offsets[n+1]) of the two lists; total  ->  counts int32[total], cum int32[total], err int32[1].  The call zeroes
 * err first; the host reads it after a stream synchronisation.
 * For an instance whose slice [lo, hi) passes list_range of gp_rle_scan.h (0 <= lo < hi <= total) and has hi - lo == runs:
 *     cum[lo + r] = the position of its r-th transition;  cum[hi - 1] = H*W
 *     counts[i] = cum[i] - cum[i-1], and the first is cum[lo]
 * Any other instance writes nothing and puts n + 1 into err.  No index derived from the data is used unchecked against the
 * slice.  By construction cum is what gpi_rle_scan leaves for counts: what takes masks = (cum, offsets) takes these lists.
 * Shape: grid (chunk, instance); a workgroup's base rank is the sum of the earlier chunks' counts from the workspace (at
 * most 1 024 chunks), the previous transition's position their maximum; inside the chunk a block scan of the transition flags;
 * the first pixel of a chunk compares with the last pixel of the previous chunk. */
int gpg_write_runs(const unsigned char* cls, int N, int H, int W, int which, const void* workspace, const int* offsets, int total,
                   int* counts, int* cum, int* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_GTINFO_H */
