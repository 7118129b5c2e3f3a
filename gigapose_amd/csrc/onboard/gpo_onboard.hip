// libgigapose_onboard.so (C-ABI: include/gigapose_onboard.h): object onboarding, the stage in front of set_template_data -- the
// RGBA renders of an object (u8, interleaved, as a PNG decoder yields them) become the cropped, normalised templates on the GPU.
//   reference: TemplateData.load_template    src/custom_megapose/template_dataset.py:66-83   (PIL getbbox per render)
//              TemplateSet.__getitem__       src/dataloader/template.py:55-81                 (CropResizePad per render + normalize)
//              CropResizePad.__call__        src/utils/crop.py:11-61
// gpo_alpha_boxes is getbbox() on the alpha channel: a pure read of H*W*4 bytes per render, min / max of the columns and rows that
// hold alpha > 0.  gpo_crop_templates is the crop skeleton of gp_crop_geom.h, shared with the detection crops, over the interleaved
// u8 pixel as its source: the four channels of a source pixel are ONE 4-byte load, the mask keeps its 256 levels and the colour
// is not multiplied by it.  So the three routes agree on every pixel.  The host-side plumbing is gp_front.h's.
// This library links no object of libgigapose_hip.so or libgigapose_ingest.so and exports only gpo_* names.
#include <limits.h>

#include "gigapose_onboard.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpo
#include "../gp_front.h"
#include "../gp_crop_geom.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTargetBlocks = 2048;   // 8 workgroups on each of 256 CUs
constexpr int kBatch = 4;             // loads a thread has in flight
constexpr int kMinLoads = kBatch;     // loads per thread below which another band is not worth its atomics

// The accumulators ARE the boxes: (W, H, 0, 0) is the neutral element of (min, min, max, max) over columns < W, rows < H and
// x1, y1 >= 1, so a template without alpha is still (W, H, 0, 0) when alpha_box_finish looks at it.
__global__ void alpha_box_init(long long* __restrict__ boxes, int N, int H, int W)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    boxes[4 * n + 0] = W;
    boxes[4 * n + 1] = H;
    boxes[4 * n + 2] = 0;
    boxes[4 * n + 3] = 0;
}

__global__ void alpha_box_finish(long long* __restrict__ boxes, int N, int* __restrict__ err)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || boxes[4 * n + 2] != 0) return;
    boxes[4 * n + 0] = 0;   // fully transparent: getbbox() is None
    boxes[4 * n + 1] = 0;
    boxes[4 * n + 3] = 0;
    atomicExch(err, n + 1);
}

// bit k set <=> pixel k of the load has alpha > 0 (the alpha byte is the word's highest)
__device__ __forceinline__ unsigned alpha_bits(uint32_t w) { return w > 0x00ffffffu; }
__device__ __forceinline__ unsigned alpha_bits(const uint4& w)
{
    return (unsigned)(w.x > 0x00ffffffu) | (unsigned)(w.y > 0x00ffffffu) << 1 | (unsigned)(w.z > 0x00ffffffu) << 2 |
           (unsigned)(w.w > 0x00ffffffu) << 3;
}

template <typename V> __device__ __forceinline__ V no_alpha();
template <> __device__ __forceinline__ uint32_t no_alpha<uint32_t>() { return 0u; }
template <> __device__ __forceinline__ uint4 no_alpha<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }

// grid (bands, N): a workgroup reads rows [band * rows_per_band, ...) of template n as one contiguous run of loads of type V
// (uint4 = four pixels when W % 4 == 0 and the base is 16-byte aligned, uint32_t = one pixel otherwise).  A thread walks the run
// with stride 256 and carries (row, column) of its load along, so no pixel costs a division.
template <typename V>
__global__ __launch_bounds__(kThreads) void alpha_box_kernel(const uint32_t* __restrict__ rgba, int H, int W, int rows_per_band,
                                                             long long* __restrict__ boxes)
{
    constexpr int kPix = sizeof(V) / 4;
    __shared__ int part[kWaves][4];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * rows_per_band;
    const int r1 = r0 + rows_per_band < H ? r0 + rows_per_band : H;
    if (r0 >= r1) return;   // uniform over the block
    const int vw = W / kPix;                                   // loads per row
    const unsigned nvec = (unsigned)(r1 - r0) * (unsigned)vw;   // < 2^31
    const V* src = reinterpret_cast<const V*>(rgba + (size_t)n * H * W + (size_t)r0 * W);
    const int step_r = kThreads / vw, step_c = kThreads % vw;
    int row = tid / vw, col = tid - row * vw;
    int minx = INT_MAX, maxx = -1, miny = INT_MAX, maxy = -1;
    for (unsigned v0 = tid; v0 < nvec; v0 += kBatch * kThreads) {
        V w[kBatch];   // all loads of a batch are issued before the first is looked at
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const unsigned v = v0 + k * kThreads;
            w[k] = v < nvec ? src[v] : no_alpha<V>();
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const unsigned m = alpha_bits(w[k]);
            if (m) {
                const int x = col * kPix;
                const int lo = x + __ffs(m) - 1, hi = x + 31 - __clz(m);
                minx = lo < minx ? lo : minx;
                maxx = hi > maxx ? hi : maxx;
                miny = row < miny ? row : miny;
                maxy = row;   // rows only grow along a thread's walk
            }
            row += step_r;
            col += step_c;
            if (col >= vw) {
                col -= vw;
                ++row;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        minx = min(minx, __shfl_xor(minx, off));
        maxx = max(maxx, __shfl_xor(maxx, off));
        miny = min(miny, __shfl_xor(miny, off));
        maxy = max(maxy, __shfl_xor(maxy, off));
    }
    if (lane == 0) {
        part[wave][0] = minx;
        part[wave][1] = maxx;
        part[wave][2] = miny;
        part[wave][3] = maxy;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            minx = min(minx, part[w][0]);
            maxx = max(maxx, part[w][1]);
            miny = min(miny, part[w][2]);
            maxy = max(maxy, part[w][3]);
        }
        if (maxx >= 0) {   // this band saw alpha: one atomic per coordinate
            long long* box = boxes + 4 * (size_t)n;
            atomicMin(box + 0, (long long)minx);
            atomicMin(box + 1, (long long)(r0 + miny));
            atomicMax(box + 2, (long long)(maxx + 1));
            atomicMax(box + 3, (long long)(r0 + maxy + 1));
        }
    }
}

// the interleaved-u8 source: R | G << 8 | B << 16 | A << 24 in one word
struct RgbaSource {
    const uint32_t* img;
    int W;
    __device__ __forceinline__ void fetch(int sy, int sx, float (&v)[3], float& m) const
    {
        const uint32_t px = img[(size_t)sy * W + sx];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)((px >> (8 * c)) & 0xffu) / 255.0f;   // rgba / 255 (template_dataset.py:103)
        m = (float)(px >> 24) / 255.0f;
    }
};

// grid (target rows, N); block = 256 threads, thread = output column
__global__ __launch_bounds__(kThreads) void crop_templates_kernel(const uint32_t* __restrict__ rgba, const long long* __restrict__ boxes,
                                                                  int H, int W, int target, float m0, float m1, float m2, float s0,
                                                                  float s1, float s2, float* __restrict__ rgb,
                                                                  float* __restrict__ mask, float* __restrict__ M,
                                                                  int* __restrict__ err)
{
    __shared__ CropGeom g;
    const int n = blockIdx.y, y = blockIdx.x;
    if (!crop_block_enter(g, boxes, n, y, H, W, target, false, M, err)) return;
    const RgbaSource src = {rgba + (size_t)n * H * W, W};
    crop_row_normalized(g, n, y, target, src, m0, m1, m2, s0, s1, s2, rgb, mask);
}

}  // namespace

extern "C" {

int gpo_abi_version(void) { return 1; }

int gpo_alpha_boxes(const uint8_t* rgba, int N, int H, int W, long long* boxes, int* err_flag, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W), "gpo_alpha_boxes: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(rgba && boxes && err_flag, "gpo_alpha_boxes: null pointer");
    GPF_REQUIRE(((uintptr_t)rgba & 3) == 0, "gpo_alpha_boxes: rgba is not 4-byte aligned (one pixel is one word)");
    const hipStream_t s = (hipStream_t)stream;
    const bool vec = (W & 3) == 0 && ((uintptr_t)rgba & 15) == 0;   // then every template and every row starts 16-byte aligned
    const int vw = vec ? W / 4 : W;
    const int min_rows = (kMinLoads * kThreads + vw - 1) / vw;
    int bands = (kTargetBlocks + N - 1) / N;
    int rows_per_band = (H + bands - 1) / bands;
    if (rows_per_band < min_rows) rows_per_band = min_rows;
    bands = (H + rows_per_band - 1) / rows_per_band;
    const dim3 small((N + kThreads - 1) / kThreads);
    const uint32_t* px = reinterpret_cast<const uint32_t*>(rgba);
    hipLaunchKernelGGL(alpha_box_init, small, dim3(kThreads), 0, s, boxes, N, H, W);
    GPF_CHECK_LAUNCH("gpo_alpha_boxes");
    if (vec) hipLaunchKernelGGL(alpha_box_kernel<uint4>, dim3(bands, N), dim3(kThreads), 0, s, px, H, W, rows_per_band, boxes);
    else hipLaunchKernelGGL(alpha_box_kernel<uint32_t>, dim3(bands, N), dim3(kThreads), 0, s, px, H, W, rows_per_band, boxes);
    GPF_CHECK_LAUNCH("gpo_alpha_boxes");
    hipLaunchKernelGGL(alpha_box_finish, small, dim3(kThreads), 0, s, boxes, N, err_flag);
    GPF_CHECK_LAUNCH("gpo_alpha_boxes");
    return GPF_OK;
}

int gpo_crop_templates(const uint8_t* rgba, const long long* boxes, int N, int H, int W, int target, const float* mean3_host,
                       const float* std3_host, float* rgb, float* mask, float* M, int* err_flag, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W) && target > 0 && target <= 4096,
                "gpo_crop_templates: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31, 0 < target <= 4096)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(rgba && boxes && mean3_host && std3_host && rgb && mask && M && err_flag, "gpo_crop_templates: null pointer");
    GPF_REQUIRE(((uintptr_t)rgba & 3) == 0, "gpo_crop_templates: rgba is not 4-byte aligned (one pixel is one word)");
    hipLaunchKernelGGL(crop_templates_kernel, dim3(target, N), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(rgba), boxes, H, W, target, mean3_host[0], mean3_host[1], mean3_host[2],
                       std3_host[0], std3_host[1], std3_host[2], rgb, mask, M, err_flag);
    GPF_CHECK_LAUNCH("gpo_crop_templates");
    return GPF_OK;
}

}  // extern "C"
