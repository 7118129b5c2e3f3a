/*
 * gigapose_onboard.h -- C-ABI of libgigapose_onboard.so: object onboarding on MI355X (gfx950), the stage in front of
 * GigaPose.set_template_data.  The RGBA renders of an object (u8, as a PNG decoder yields them) go to the GPU as they are; the
 * box of every render is taken from its alpha channel and the normalised crops, masks and crop transforms are written by one
 * gather.  Reference: TemplateData.load_template (src/custom_megapose/template_dataset.py:66-83, PIL getbbox per render) and
 * TemplateSet.__getitem__ (src/dataloader/template.py:55-81, CropResizePad one render at a time on the CPU + normalize).
 * The hot-path interface is gigapose_hip.h / libgigapose_hip.so and the detection ingest is gigapose_ingest.h /
 * libgigapose_ingest.so; this library is separate from both and links none of their objects.
 *
 * Conventions (those of gigapose_ingest.h)
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all buffers, kernels never allocate;
 *     inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpo_last_error() returns a thread-local message
 *     for the last failure;
 *   - err_flag: one int32 on the device, zeroed by the caller.  A bad template n stores n + 1 there (if several are bad, one
 *     of them); the others are processed.
 *
 * Render format: rgba u8 (N,H,W,4), interleaved and contiguous -- np.array(PIL image) of an RGBA PNG, stacked.  One pixel is
 * one 4-byte word (R in the lowest byte, A in the highest), so `rgba` must be 4-byte aligned.
 * Limits: N <= 65535 per call (gigapose_amd/onboard.py chunks), H*W < 2^31, H*W*4*N is addressed with size_t, target <= 4096.
 */
#ifndef GIGAPOSE_ONBOARD_H
#define GIGAPOSE_ONBOARD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpo_abi_version(void);
const char* gpo_last_error(void);

/* PIL.Image.getbbox() of an RGBA image as load_template calls it (template_dataset.py:76; Pillow >= 10, where alpha_only=True
 * is the default): boxes[n] = (x0, y0, x1, y1) with x0 / y0 the least column / row that holds a pixel of alpha > 0 and
 * x1 / y1 the greatest such column / row + 1.  The colour channels are ignored.
 * The call initialises `boxes` itself: what the buffer held before does not matter.
 * Bad: a fully transparent template (getbbox() returns None and the reference fails at box[2]).  Its box is written as
 * 0,0,0,0 and err_flag is set.
 * Not built: the reference's "zero area -> full frame" branch (template_dataset.py:78-82).  A box that getbbox() returns has
 * x1 > x0 and y1 > y0, so the branch cannot be reached.
 * Several workgroups per template, each over a band of rows: 16 bytes (four pixels) per lane when W is a multiple of 4 and
 * `rgba` is 16-byte aligned, one pixel per lane otherwise; min / max in the wave, then in the workgroup, then at most one
 * integer atomic per box coordinate and workgroup -- the result does not depend on the order. */
int gpo_alpha_boxes(const uint8_t* rgba, int N, int H, int W, long long* boxes /* (N,4) xyxy */, int* err_flag, void* stream);

/* TemplateSet.__getitem__ (template.py:64-70) as one gather: rgba / 255, CropResizePad (src/utils/crop.py:11-61) on the four
 * channels, (x - mean) / std on the first three.
 *   rgba (N,H,W,4) u8, boxes (N,4) int64 xyxy, mean3/std3: HOST arrays of 3 floats
 *   -> rgb (N,3,target,target), mask (N,target,target) = the cropped alpha / 255 (256 levels: NOT binarised, and the colour is
 *      NOT multiplied by it -- unlike the detection crop), M (N,3,3).  Padding pixels give (0 - mean) / std and mask 0.
 * The source-index arithmetic is that of gp_preprocess_detections (gigapose_hip.h), shared through csrc/gp_crop_geom.h.
 * Bad: an empty / out-of-frame box (0,0,0,0 from gpo_alpha_boxes included), or a box whose short side scales to 0 pixels
 * (the reference raises inside F.interpolate).  A bad template leaves ITS rgb / mask / M untouched. */
int gpo_crop_templates(const uint8_t* rgba, const long long* boxes, int N, int H, int W, int target, const float* mean3_host,
                       const float* std3_host, float* rgb, float* mask, float* M, int* err_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_ONBOARD_H */
