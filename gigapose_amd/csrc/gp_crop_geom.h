// The crop kernels' common part, shared by gp_crop.hip (dense masks), ingest/gpi_ingest.hip (run-length masks) and
// onboard/gpo_onboard.hip (RGBA renders).  Header only; written ONCE: the translation units must never disagree on a pixel.
//   - the source-index arithmetic: both resizes of CropResizePad.__call__ (src/utils/crop.py:11-61) are nearest-neighbour, so
//     output pixel (y, x) maps to one source pixel through the composed index maps below -- exactly the integer / float
//     arithmetic of ATen's CPU nearest kernels as measured on torch 2.10 (oracle/crop_numpy.py states it, and
//     tests/test_crop_aten_sweep.py holds that statement to ATen itself);
//   - the kernel skeleton, grid (target rows, items), block = 256 threads, thread = output column: crop_block_enter (geometry,
//     error flag or M, barrier) and crop_row_normalized (the row loop over a pixel source, Normalize's stores).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

struct CropGeom {
    int x0, y0, cw, ch;      // crop window after the border clamp
    int h1, w1;              // size after the first resize
    int pad_t, pad_l, hp, wp;
    float inv1;              // (float)(1.0 / scale): source-index scale of the first resize
    int mode1y, mode1x;      // 0 identity, 1 dst >> 1, 2 min(floorf(dst * inv1), in - 1)
    float s2y, s2x;          // in/out scales of the final resize
    int mode2y, mode2x;
    float scale32;
    int bad;
};

// ATen's CPU upsample_nearest2d has two kernels and picks one per call, for both dimensions: the one whose nearest_idx
// (UpSample.h) returns dst for out == in and dst >> 1 for out == 2 * in runs only while out_h + out_w <= 128 (or on a
// channels-last input of more than 3 channels: never a slice of an NCHW frame); the generic kernel floors every index.
// The two differ under a scale_factor that is not exactly 1 or 2.
constexpr int kAtenVectorizedMaxHW = 128;
__device__ __forceinline__ int resize_mode(int out, int in, bool shortcuts)
{
    return !shortcuts ? 2 : (out == in ? 0 : (out == 2 * in ? 1 : 2));
}

// source index of one dimension: the shortcuts where resize_mode granted them, else min(floorf(dst * scale), in - 1)
__device__ __forceinline__ int nearest_src(int dst, int in, int mode, float scale)
{
    if (mode == 0) return dst;
    if (mode == 1) return dst >> 1;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

__device__ void make_geom(const long long* box, int H, int W, int target, CropGeom& g)
{
    const long long bx0 = box[0], by0 = box[1], bx1 = box[2], by1 = box[3];
    g.bad = !(0 <= bx0 && bx0 < bx1 && 0 <= by0 && by0 < by1 && bx0 < W && by0 < H && bx1 - bx0 < (1 << 24) &&
              by1 - by0 < (1 << 24));
    if (g.bad) return;
    g.x0 = (int)bx0;
    g.y0 = (int)by0;
    const int bw = (int)(bx1 - bx0), bh = (int)(by1 - by0);
    // crop.py:20, `target_size / int32_tensor`: Tensor.__rtruediv__ is reciprocal() * target, TWO float32 roundings (built
    // with -ffp-contract=off -fno-fast-math: a true division, then a multiply)
    g.scale32 = (1.0f / (float)(bw > bh ? bw : bh)) * (float)target;
    const double scale = (double)g.scale32;                            // .item()
    g.cw = (int)((bx1 < W ? bx1 : W) - bx0);                            // slicing clamps (crop.py:31)
    g.ch = (int)((by1 < H ? by1 : H) - by0);
    g.h1 = (int)floor((double)g.ch * scale);                           // F.interpolate(scale_factor): floor(in * s)
    g.w1 = (int)floor((double)g.cw * scale);
    if (g.h1 <= 0 || g.w1 <= 0) { g.bad = 1; return; }
    g.inv1 = (float)(1.0 / scale);
    const bool short1 = g.h1 + g.w1 <= kAtenVectorizedMaxHW;
    g.mode1y = resize_mode(g.h1, g.ch, short1);
    g.mode1x = resize_mode(g.w1, g.cw, short1);
    g.pad_t = g.pad_l = 0;
    g.hp = g.h1;
    g.wp = g.w1;
    if (g.w1 != g.h1) {                                                // crop.py:37-47
        g.pad_t = (target - g.h1) >= 0 ? (target - g.h1) / 2 : -((g.h1 - target + 1) / 2);  // Python floor division
        int pad_b = target - g.h1 - g.pad_t;
        if (pad_b < 0) pad_b = 0;
        g.pad_l = (target - g.w1) >= 0 ? (target - g.w1) / 2 : -((g.w1 - target + 1) / 2);
        if (g.pad_l < 0) g.pad_l = 0;
        const int pad_r = target - g.w1 - g.pad_l;
        g.hp = g.h1 + g.pad_t + pad_b;
        g.wp = g.w1 + g.pad_l + pad_r;
    }
    if (g.hp <= 0 || g.wp <= 0) { g.bad = 1; return; }
    g.mode2y = resize_mode(target, g.hp, true);                        // in / out is exactly 1 or 0.5 there: the shortcuts
    g.mode2x = resize_mode(target, g.wp, true);                        // and the floor agree, whichever kernel runs
    g.s2y = (float)g.hp / (float)target;                               // scales not given: in / out
    g.s2x = (float)g.wp / (float)target;
}

// source pixel of output (y, x) inside the frame, or -1 when it falls in the zero padding
__device__ __forceinline__ int source_y(const CropGeom& g, int y)
{
    const int yp = nearest_src(y, g.hp, g.mode2y, g.s2y) - g.pad_t;
    if (yp < 0 || yp >= g.h1) return -1;
    return g.y0 + nearest_src(yp, g.ch, g.mode1y, g.inv1);
}
__device__ __forceinline__ int source_x(const CropGeom& g, int x)
{
    const int xp = nearest_src(x, g.wp, g.mode2x, g.s2x) - g.pad_l;
    if (xp < 0 || xp >= g.w1) return -1;
    return g.x0 + nearest_src(xp, g.cw, g.mode1x, g.inv1);
}

__device__ __forceinline__ void write_M(const CropGeom& g, float* M)
{
    // M = M_resize_pad @ M_crop (crop.py:26-49): [[s, 0, s*(-x0) + pad_l], [0, s, s*(-y0) + pad_t], [0, 0, 1]]
    const float s = g.scale32;
    const float pl = g.w1 != g.h1 ? (float)g.pad_l : 0.f, pt = g.w1 != g.h1 ? (float)g.pad_t : 0.f;
    M[0] = s; M[1] = 0.f; M[2] = s * (-(float)g.x0) + pl;
    M[3] = 0.f; M[4] = s; M[5] = s * (-(float)g.y0) + pt;
    M[6] = 0.f; M[7] = 0.f; M[8] = 1.f;
}

// Block entry of a crop kernel, called by every thread: thread 0 builds the geometry of item d from its box, `also_bad` (thread
// 0's value counts: a frame id out of range, an invalid run list) marks the item bad as well, and the block of row 0 reports --
// d + 1 into *err for a bad item, which is then left unwritten, or the item's M.  Returns whether the block proceeds.
__device__ __forceinline__ bool crop_block_enter(CropGeom& g, const long long* __restrict__ boxes, int d, int y, int H, int W,
                                                 int target, bool also_bad, float* __restrict__ M, int* __restrict__ err)
{
    if (threadIdx.x == 0) {
        make_geom(boxes + 4 * d, H, W, target, g);
        if (also_bad) g.bad = 1;
        if (y == 0) {
            if (g.bad) atomicExch(err, d + 1);
            else write_M(g, M + 9 * d);
        }
    }
    __syncthreads();
    return !g.bad;
}

// rgb / 255.0 * mask (train.py:83,107) of pixel o of a planar u8 frame: the colour of the detection crops
__device__ __forceinline__ void masked_rgb(const uint8_t* __restrict__ frame, size_t plane, size_t o, float m, float (&v)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((float)frame[c * plane + o] / 255.0f) * m;
}

// Row y of item d: every output pixel takes colour and mask of its source pixel from `src.fetch(sy, sx, v, m)` -- the zero
// padding has none and keeps v = 0, m = 0 -- and stores torchvision's Normalize of the colour, (v - mean) / std, and the mask.
template <typename Source>
__device__ __forceinline__ void crop_row_normalized(const CropGeom& g, int d, int y, int target, const Source& src, float m0,
                                                    float m1, float m2, float s0, float s1, float s2, float* __restrict__ out_rgb,
                                                    float* __restrict__ out_mask)
{
    const int sy = source_y(g, y);
    const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    for (int x = threadIdx.x; x < target; x += blockDim.x) {
        const int sx = sy < 0 ? -1 : source_x(g, x);
        float m = 0.f;
        float v[3] = {0.f, 0.f, 0.f};
        if (sx >= 0) src.fetch(sy, sx, v, m);
        const size_t po = (size_t)y * target + x, tt = (size_t)target * target;
#pragma unroll
        for (int c = 0; c < 3; ++c) out_rgb[((size_t)d * 3 + c) * tt + po] = (v[c] - mean[c]) / stdv[c];
        out_mask[(size_t)d * tt + po] = m;
    }
}

}  // namespace
