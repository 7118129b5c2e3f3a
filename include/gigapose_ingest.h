/*
 * gigapose_ingest.h -- C-ABI of libgigapose_ingest.so: the stage BEFORE the GigaPose hot path on MI355X (gfx950).
 * Camera frames (u8) and CNOS detections whose masks are still run-length lists go to the GPU as they are; the masks are
 * decoded while the crops are taken.  Reference: GigaPoseTestSet.add_detections / collate_fn (src/dataloader/test.py:205-318)
 * with process_real (src/dataloader/train.py:80-123), which expand every mask to a dense H x W array on the CPU.
 * The hot-path interface is gigapose_hip.h / libgigapose_hip.so; this library is separate from it and links none of its objects.
 *
 * Conventions (those of gigapose_hip.h)
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all buffers, kernels never allocate;
 *     inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpi_last_error() returns a thread-local message
 *     for the last failure;
 *   - err_flag: one int32 on the device, zeroed by the caller.  A bad detection d leaves ITS outputs untouched and stores
 *     d + 1 there (if several are bad, one of them); the others are processed.
 *
 * Mask format: uncompressed COCO run-length encoding, exactly what mask_to_rle writes (src/utils/mask.py:9-27):
 *   - size = [H, W];
 *   - counts holds the lengths of alternating runs of 0 and 1 over the mask flattened COLUMN-major: pixel (y, x) has
 *     index p = x*H + y;
 *   - the first run is zeros and may have length 0;
 *   - the counts sum to H*W;
 *   - with cum the inclusive prefix sums, pixel p lies in run j = #{i : cum[i] <= p}, and its value is j & 1.
 * The lists of D detections are concatenated: counts i32[total], detection d owns [offsets[d], offsets[d+1]), offsets i32[D+1].
 * Compressed string counts (pycocotools' byte coding) are not handled.
 * Limits: H*W < 2^31, total < 2^30, D <= 65535.
 */
#ifndef GIGAPOSE_INGEST_H
#define GIGAPOSE_INGEST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpi_abi_version(void);
const char* gpi_last_error(void);

/* Per-detection inclusive prefix sum: cum[i] = counts[offsets[d]] + ... + counts[i] for i in detection d's slice.
 * One workgroup per detection (a wave scan plus an LDS carry over chunks of the list): any list length.
 * A detection is BAD when its slice is empty or leaves [0, total], a count is negative, or the counts do not sum to exactly
 * H*W (bop_toolkit's pycoco_utils.rle_to_binary_mask, called at src/dataloader/test.py:238, fails on its reshape there).  A bad detection is marked inside cum (its last entry is -1) so that the calls below skip it. */
int gpi_rle_scan(const int* counts, const int* offsets, int total, int D, int H, int W, int* cum, int* err_flag, void* stream);

/* gp_preprocess_detections (gigapose_hip.h; process_real + normalize, src/dataloader/train.py:80-123,
 * src/dataloader/test.py:295-315, crop: src/utils/crop.py:11-61) with the mask value of each gathered source pixel taken from
 * the runs instead of a dense (D,H,W) array; the results are bit-identical to it.
 *   rgb (n_img,3,H,W) u8 full frames, cum / offsets from gpi_rle_scan, boxes (D,4) int64 xyxy, im_id (D) int32 frame of each
 *   detection, mean3/std3: HOST arrays of 3 floats -> tar_img (D,3,target,target), tar_mask (D,target,target), M (D,3,3).
 * Bad: an empty / out-of-frame box or a frame id outside [0, n_img) (as gp_preprocess_detections), or a list gpi_rle_scan
 * marked bad. */
int gpi_preprocess_detections_rle(const uint8_t* rgb, const int* cum, const int* offsets, int total, const long long* boxes,
                                  const int* im_id, int n_img, int D, int H, int W, int target, const float* mean3_host,
                                  const float* std3_host, float* tar_img, float* tar_mask, float* M, int* err_flag, void* stream);

/* The dense masks (D,H,W) f32 {0,1} (the reference keeps them as scene_obs.binary_masks, src/dataloader/test.py:238-241).
 * A detection gpi_rle_scan marked bad is left untouched. */
int gpi_rle_decode(const int* cum, const int* offsets, int total, int D, int H, int W, float* masks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_INGEST_H */
