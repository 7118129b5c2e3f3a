// Detection pre-processing on the GPU: the step immediately before the hot path.
//   reference: CropResizePad.__call__            src/utils/crop.py:11-61
//              process_real (rgb/255 * mask)     src/dataloader/train.py:80-123
//              collate_fn normalize(real_data.rgb) src/dataloader/test.py:295-315, configs/data/transform.yaml:1-12
// The reference runs this per detection in Python on the CPU (DataLoader workers): slice, nearest
// F.interpolate(scale_factor), F.pad, nearest F.interpolate(size) -- four passes and three temporaries per
// detection.  Both resizes are nearest-neighbour, so the whole chain is ONE gather: output pixel (y, x) ->
// index in the padded image -> index in the scaled crop -> source pixel.  The kernels below compose the index
// maps with exactly the integer/float arithmetic of ATen's nearest kernels (restated in oracle/crop_numpy.py,
// which is pinned bit-exactly to the reference golden) and write each output pixel once: HBM-bound, coalesced
// stores, one block per output row.
#include <math.h>

#include "gp_common.h"
#include "gp_crop_geom.h"

namespace {

// grid (target rows, D); block = 256 threads, thread = output column
__global__ __launch_bounds__(256) void crop_resize_pad_kernel(const float* __restrict__ images,
                                                               const long long* __restrict__ boxes, int C, int H, int W,
                                                               int target, float* __restrict__ out, float* __restrict__ M,
                                                               int* __restrict__ err)
{
    __shared__ CropGeom g;
    const int d = blockIdx.y, y = blockIdx.x;
    if (!crop_block_enter(g, boxes, d, y, H, W, target, false, M, err)) return;
    const int sy = source_y(g, y);
    for (int x = threadIdx.x; x < target; x += blockDim.x) {
        const int sx = sy < 0 ? -1 : source_x(g, x);
        for (int c = 0; c < C; ++c) {
            float v = 0.f;
            if (sx >= 0) v = images[(((size_t)d * C + c) * H + sy) * W + sx];
            out[(((size_t)d * C + c) * target + y) * target + x] = v;
        }
    }
}

// the dense source: masks[d][sy][sx] and the frame's pixel times it
struct DenseSource {
    const uint8_t* frame;
    const float* mask;
    int W;
    size_t plane;
    __device__ __forceinline__ void fetch(int sy, int sx, float (&v)[3], float& m) const
    {
        const size_t o = (size_t)sy * W + sx;
        m = mask[o];
        masked_rgb(frame, plane, o, m, v);
    }
};

__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ rgb, const float* __restrict__ masks,
                                                          const long long* __restrict__ boxes, const int* __restrict__ im_id,
                                                          int n_img, int H, int W, int target, float m0, float m1, float m2,
                                                          float s0, float s1, float s2, float* __restrict__ tar_img,
                                                          float* __restrict__ tar_mask, float* __restrict__ M,
                                                          int* __restrict__ err)
{
    __shared__ CropGeom g;
    __shared__ int img;
    const int d = blockIdx.y, y = blockIdx.x;
    if (threadIdx.x == 0) img = im_id[d];
    if (!crop_block_enter(g, boxes, d, y, H, W, target, threadIdx.x == 0 && (img < 0 || img >= n_img), M, err)) return;
    const size_t plane = (size_t)H * W;
    const DenseSource src = {rgb + (size_t)img * 3 * plane, masks + (size_t)d * plane, W, plane};
    crop_row_normalized(g, d, y, target, src, m0, m1, m2, s0, s1, s2, tar_img, tar_mask);
}

}  // namespace

extern "C" {

int gp_crop_resize_pad(const float* images, const long long* boxes, int D, int C, int H, int W, int target, float* out,
                       float* M, int* err_flag, void* stream)
{
    GP_REQUIRE(D >= 0 && C > 0 && H > 0 && W > 0 && target > 0 && target <= 4096, "gp_crop_resize_pad: bad sizes");
    if (D == 0) return GP_OK;
    GP_REQUIRE(images && boxes && out && M && err_flag, "gp_crop_resize_pad: null pointer");
    GpProfScope prof(GP_PROF_OTHER, 0.0, (hipStream_t)stream);
    hipLaunchKernelGGL(crop_resize_pad_kernel, dim3(target, D), dim3(256), 0, (hipStream_t)stream, images, boxes, C, H, W,
                       target, out, M, err_flag);
    GP_CHECK_LAUNCH("gp_crop_resize_pad");
    return GP_OK;
}

int gp_preprocess_detections(const uint8_t* rgb, const float* masks, const long long* boxes, const int* im_id, int n_img,
                             int D, int H, int W, int target, const float* mean3_host, const float* std3_host,
                             float* tar_img, float* tar_mask, float* M, int* err_flag, void* stream)
{
    GP_REQUIRE(D >= 0 && n_img > 0 && H > 0 && W > 0 && target > 0 && target <= 4096, "gp_preprocess_detections: bad sizes");
    if (D == 0) return GP_OK;
    GP_REQUIRE(rgb && masks && boxes && im_id && mean3_host && std3_host && tar_img && tar_mask && M && err_flag,
               "gp_preprocess_detections: null pointer");
    GpProfScope prof(GP_PROF_OTHER, 0.0, (hipStream_t)stream);
    hipLaunchKernelGGL(preprocess_kernel, dim3(target, D), dim3(256), 0, (hipStream_t)stream, rgb, masks, boxes, im_id,
                       n_img, H, W, target, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1],
                       std3_host[2], tar_img, tar_mask, M, err_flag);
    GP_CHECK_LAUNCH("gp_preprocess_detections");
    return GP_OK;
}

}  // extern "C"
