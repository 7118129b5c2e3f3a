// Source-index arithmetic of the detection crop, shared by gp_crop.hip (dense masks) and ingest/gpi_ingest.hip (run-length
// masks): both resizes of CropResizePad.__call__ (src/utils/crop.py:11-61) are nearest-neighbour, so output pixel (y, x) maps
// to one source pixel through the composed index maps below -- exactly the integer / float arithmetic of ATen's nearest
// kernels, restated in oracle/crop_numpy.py.  Written ONCE: the two translation units must never disagree on a pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

struct CropGeom {
    int x0, y0, cw, ch;      // crop window after the border clamp
    int h1, w1;              // size after the first resize
    int pad_t, pad_l, hp, wp;
    float inv1;              // (float)(1.0 / scale): source-index scale of the first resize
    int mode1y, mode1x;      // 0 identity, 1 dst >> 1, 2 floorf(dst * inv1)
    float s2y, s2x;          // in/out scales of the final resize
    int mode2y, mode2x;
    float scale32;
    int bad;
};

__device__ __forceinline__ int resize_mode(int out, int in) { return out == in ? 0 : (out == 2 * in ? 1 : 2); }

// ATen nearest_idx (UpSample.h): identity / >>1 shortcuts, else min(floorf(dst * scale), in - 1)
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
    g.scale32 = (float)target / (float)(bw > bh ? bw : bh);            // crop.py:20 (float32 tensor division)
    const double scale = (double)g.scale32;                            // .item()
    g.cw = (int)((bx1 < W ? bx1 : W) - bx0);                            // slicing clamps (crop.py:31)
    g.ch = (int)((by1 < H ? by1 : H) - by0);
    g.h1 = (int)floor((double)g.ch * scale);                           // F.interpolate(scale_factor): floor(in * s)
    g.w1 = (int)floor((double)g.cw * scale);
    if (g.h1 <= 0 || g.w1 <= 0) { g.bad = 1; return; }
    g.inv1 = (float)(1.0 / scale);
    g.mode1y = resize_mode(g.h1, g.ch);
    g.mode1x = resize_mode(g.w1, g.cw);
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
    g.mode2y = resize_mode(target, g.hp);
    g.mode2x = resize_mode(target, g.wp);
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

}  // namespace
