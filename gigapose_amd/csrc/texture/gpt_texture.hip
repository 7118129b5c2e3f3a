// libgigapose_texture.so (C-ABI: include/gigapose_texture.h): the colour of a rendered mesh from ONE texture image through
// per-corner UV coordinates, beside libgigapose_render.so, whose gpr_project / gpr_raster write the keys this library reads.
//   reference: src/custom_megapose/call_panda3d.py:45-95 with the mip-mapped filters of
//   src/megapose/panda3d_renderer/panda3d_scene_renderer.py:70-71
// gpt_build_mips: the image as 32-bit texels, then one launch per level of 2 x 2 rounded means.  gpt_resolve: one thread per
// pixel; perspective-correct UV at the pixel and at its right and lower neighbour, a level of detail from the squared UV
// steps (comparisons with powers of four: no logarithm), one or two bilinear samples with repeat wrapping: 4 or 8 texel loads
// of 4 bytes.  The arithmetic is spelled out in the header and restated in gigapose_testing/texture_ref.py; the two agree bit
// for bit.  The host-side plumbing is gp_front.h's; the triangle set-up, what the kernel reads out of a pixel's key (the gate,
// the centre weights, the depth) and the rounding to a byte are gp_raster_geom.h's (shared with the render and shade
// libraries).  This library links no object of the other libraries and exports only gpt_* names.
#include <math.h>

#include "gigapose_texture.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpt
#include "../gp_front.h"
#include "../gp_raster_geom.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTexture = 16384;
constexpr int kMaxLevels = 15;             // 1 + log2(16384)
constexpr double kMaxUV = 32768.0;         // GPT_MAX_UV

// the pyramid's layout, by value in the kernel arguments
struct Pyramid {
    int levels;
    int w[kMaxLevels], h[kMaxLevels];
    unsigned off[kMaxLevels];              // first texel of the level; the whole pyramid holds < 2^29 texels
};

bool texture_size_ok(int Ht, int Wt) { return Ht >= 1 && Wt >= 1 && Ht <= kMaxTexture && Wt <= kMaxTexture; }

size_t layout(int Ht, int Wt, Pyramid& p)
{
    size_t total = 0;
    int l = 0, h = Ht, w = Wt;
    for (;; ++l) {
        p.w[l] = w;
        p.h[l] = h;
        p.off[l] = (unsigned)total;
        total += (size_t)h * (size_t)w;
        if (h == 1 && w == 1) break;
        h = h > 1 ? h >> 1 : 1;
        w = w > 1 ? w >> 1 : 1;
    }
    p.levels = l + 1;
    for (int k = l + 1; k < kMaxLevels; ++k) p.w[k] = p.h[k] = 1, p.off[k] = p.off[l];
    return total;
}

// grid (ceil(Ht*Wt / 256)): thread = texel
__global__ __launch_bounds__(kThreads) void pack_kernel(const uint8_t* __restrict__ rgb, unsigned texels, uint32_t* __restrict__ out)
{
    const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (i >= texels) return;
    const uint8_t* p = rgb + 3 * (size_t)i;
    out[i] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | 0xff000000u;
}

// grid (ceil(h*w / 256)): thread = texel of the destination level
__global__ __launch_bounds__(kThreads) void halve_kernel(const uint32_t* __restrict__ src, int sh, int sw, uint32_t* __restrict__ dst,
                                                         int h, int w)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (p >= (unsigned)h * (unsigned)w) return;
    const int i = (int)(p / (unsigned)w), j = (int)(p - (unsigned)i * (unsigned)w);
    const int i0 = min(2 * i, sh - 1), i1 = min(2 * i + 1, sh - 1), j0 = min(2 * j, sw - 1), j1 = min(2 * j + 1, sw - 1);
    const uint32_t a = src[(size_t)i0 * sw + j0], b = src[(size_t)i1 * sw + j0], c = src[(size_t)i0 * sw + j1],
                   d = src[(size_t)i1 * sw + j1];
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) o |= ((((a >> k) & 255u) + ((b >> k) & 255u) + ((c >> k) & 255u) + ((d >> k) & 255u) + 2u) >> 2) << k;
    dst[p] = o;
}

struct UV {
    double q, u, v;
};

// from the weights t_k = (double)e_k * r_k: the pixel's own are resolve_pixel's, a neighbour's come from its edge values
__device__ __forceinline__ UV uv_at(double t0, double t1, double t2, const double* cu, const double* cv)
{
    UV o;
    o.q = (t0 + t1) + t2;
    o.u = ((t0 * cu[0] + t1 * cu[1]) + t2 * cu[2]) / o.q;
    o.v = ((t0 * cv[0] + t1 * cv[1]) + t2 * cv[2]) / o.q;
    return o;
}

__device__ __forceinline__ bool within(double x, double bound) { return x >= -bound && x <= bound; }   // false for a NaN

// |u|, |v| <= 2 * kMaxUV: |s| <= 2^30 + 1/2, floor(s) fits an int and the wrapped indices lie in [0, W_l), [0, H_l)
__device__ __forceinline__ void bilinear(const uint32_t* __restrict__ pyramid, const Pyramid& P, int l, double u, double v, double* out)
{
    const int wl = P.w[l], hl = P.h[l];
    const uint32_t* lev = pyramid + P.off[l];
    const double s = u * (double)wl - 0.5, t = (1.0 - v) * (double)hl - 0.5;
    const double fs = floor(s), ft = floor(t);
    const double fx = s - fs, fy = t - ft, gx = 1.0 - fx, gy = 1.0 - fy;
    int i0 = (int)fs % wl, j0 = (int)ft % hl;
    if (i0 < 0) i0 += wl;
    if (j0 < 0) j0 += hl;
    const int i1 = i0 + 1 == wl ? 0 : i0 + 1, j1 = j0 + 1 == hl ? 0 : j0 + 1;
    const uint32_t c00 = lev[(size_t)j0 * wl + i0], c10 = lev[(size_t)j0 * wl + i1], c01 = lev[(size_t)j1 * wl + i0],
                   c11 = lev[(size_t)j1 * wl + i1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = (double)((c00 >> (8 * c)) & 255u), b = (double)((c10 >> (8 * c)) & 255u),
                     d = (double)((c01 >> (8 * c)) & 255u), e = (double)((c11 >> (8 * c)) & 255u);
        out[c] = (gx * a + fx * b) * gy + (gx * d + fx * e) * fy;
    }
}

// grid (ceil(H*W / 256), N): thread = pixel
__global__ __launch_bounds__(kThreads) void resolve_kernel(const u64* __restrict__ vis, const int* __restrict__ xy,
                                                           const float* __restrict__ depth, int V, const int* __restrict__ faces, int F,
                                                           const float* __restrict__ corner_uv, const uint32_t* __restrict__ pyramid,
                                                           Pyramid P, int H, int W, uint32_t* __restrict__ rgba, float* __restrict__ zdepth)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (p >= (unsigned)H * (unsigned)W) return;
    const size_t o = (size_t)n * H * W + p;
    uint32_t px = 0u;
    Pixel pixel;
    resolve_pixel(vis[o], p, xy + 2 * (size_t)n * V, depth + (size_t)n * V, V, faces, F, H, W, pixel, [&](const Pixel& pix) {
        const Tri& t = pix.t;
        px = 0xff000000u;
        const float* c = corner_uv + 6 * (size_t)pix.f;
        const int k1 = t.swapped ? 2 : 1, k2 = t.swapped ? 1 : 2;   // the corners go with the vertices
        const double cu[3] = {(double)c[0], (double)c[2 * k1], (double)c[2 * k2]};
        const double cv[3] = {(double)c[1], (double)c[2 * k1 + 1], (double)c[2 * k2 + 1]};
        const UV m = uv_at(pix.t0, pix.t1, pix.t2, cu, cv);
        const bool good = within(cu[0], kMaxUV) && within(cu[1], kMaxUV) && within(cu[2], kMaxUV) && within(cv[0], kMaxUV) &&
                          within(cv[1], kMaxUV) && within(cv[2], kMaxUV) && within(m.u, 2.0 * kMaxUV) && within(m.v, 2.0 * kMaxUV);
        if (good) {
            const i64 dx0 = t.x2 - t.x1, dy0 = t.y2 - t.y1, dx1 = t.x0 - t.x2, dy1 = t.y0 - t.y2, dx2 = t.x1 - t.x0, dy2 = t.y1 - t.y0;
            const UV mx = uv_at((double)(pix.e0 - 256 * dy0) * t.r0, (double)(pix.e1 - 256 * dy1) * t.r1, (double)(pix.e2 - 256 * dy2) * t.r2, cu, cv);
            const UV my = uv_at((double)(pix.e0 + 256 * dx0) * t.r0, (double)(pix.e1 + 256 * dx1) * t.r1, (double)(pix.e2 + 256 * dx2) * t.r2, cu, cv);
            const int top = P.levels - 1;
            int l0 = top;
            bool two = false;
            double w = 0.0;
            if (!(mx.q <= 0.0 || my.q <= 0.0)) {
                const double wt = (double)P.w[0], ht = (double)P.h[0];
                const double dsdx = (mx.u - m.u) * wt, dtdx = (mx.v - m.v) * ht, dsdy = (my.u - m.u) * wt, dtdy = (my.v - m.v) * ht;
                const double ax = dsdx * dsdx + dtdx * dtdx, ay = dsdy * dsdy + dtdy * dtdy;
                if (ax == ax && ay == ay) {
                    const double rho2 = ay > ax ? ay : ax;
                    if (rho2 < 1.0) {
                        l0 = 0;
                    } else {
                        double p4 = 1.0;   // 4^l0
                        l0 = 0;
                        while (l0 < top && p4 * 4.0 <= rho2) {
                            p4 = p4 * 4.0;
                            ++l0;
                        }
                        if (l0 < top) {
                            two = true;
                            w = (rho2 / p4 - 1.0) / 3.0;
                        }
                    }
                }
            }
            double A[3], B[3];
            bilinear(pyramid, P, l0, m.u, m.v, A);
            if (two) {
                bilinear(pyramid, P, l0 + 1, m.u, m.v, B);
                const double g = 1.0 - w;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) A[ch] = g * A[ch] + w * B[ch];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px |= to_byte(A[ch]) << (8 * ch);
        }
    });
    rgba[o] = px;
    zdepth[o] = pixel.z;
}

}  // namespace

extern "C" {

int gpt_abi_version(void) { return 1; }

int gpt_mip_levels(int Ht, int Wt)
{
    if (!texture_size_ok(Ht, Wt)) return 0;
    Pyramid p;
    layout(Ht, Wt, p);
    return p.levels;
}

size_t gpt_mip_texels(int Ht, int Wt)
{
    if (!texture_size_ok(Ht, Wt)) return 0;
    Pyramid p;
    return layout(Ht, Wt, p);
}

int gpt_build_mips(const uint8_t* rgb, int Ht, int Wt, uint32_t* pyramid, void* stream)
{
    GPF_REQUIRE(texture_size_ok(Ht, Wt), "gpt_build_mips: bad sizes (1 <= Ht, Wt <= 16384)");
    GPF_REQUIRE(rgb && pyramid, "gpt_build_mips: null pointer");
    GPF_REQUIRE(((uintptr_t)pyramid & 3) == 0, "gpt_build_mips: pyramid is not 4-byte aligned (one texel is one word)");
    const hipStream_t s = (hipStream_t)stream;
    Pyramid p;
    layout(Ht, Wt, p);
    const unsigned texels = (unsigned)Ht * (unsigned)Wt;   // <= 2^28
    hipLaunchKernelGGL(pack_kernel, dim3((texels + kThreads - 1) / kThreads), dim3(kThreads), 0, s, rgb, texels, pyramid);
    GPF_CHECK_LAUNCH("gpt_build_mips");
    for (int l = 1; l < p.levels; ++l) {
        const unsigned n = (unsigned)p.h[l] * (unsigned)p.w[l];
        hipLaunchKernelGGL(halve_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, pyramid + p.off[l - 1], p.h[l - 1],
                           p.w[l - 1], pyramid + p.off[l], p.h[l], p.w[l]);
        GPF_CHECK_LAUNCH("gpt_build_mips");
    }
    return GPF_OK;
}

int gpt_resolve(const unsigned long long* vis, const int* xy, const float* depth, int V, const int* faces, int F,
                const float* corner_uv, const uint32_t* pyramid, int Ht, int Wt, int N, int H, int W, uint8_t* rgba, float* zdepth,
                void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W) && V >= 0 && F >= 0, "gpt_resolve: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31, V, F >= 0)");
    GPF_REQUIRE(texture_size_ok(Ht, Wt), "gpt_resolve: bad sizes (1 <= Ht, Wt <= 16384)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && rgba && zdepth, "gpt_resolve: null pointer");
    GPF_REQUIRE(F == 0 || (xy && depth && faces && corner_uv && pyramid), "gpt_resolve: null pointer");
    GPF_REQUIRE(((uintptr_t)rgba & 3) == 0, "gpt_resolve: rgba is not 4-byte aligned (one pixel is one word)");
    GPF_REQUIRE(((uintptr_t)pyramid & 3) == 0, "gpt_resolve: pyramid is not 4-byte aligned (one texel is one word)");
    Pyramid p;
    layout(Ht, Wt, p);
    const unsigned blocks = (unsigned)(((long long)H * W + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks, N), dim3(kThreads), 0, (hipStream_t)stream, vis, xy, depth, V, faces, F, corner_uv,
                       pyramid, p, H, W, reinterpret_cast<uint32_t*>(rgba), zdepth);
    GPF_CHECK_LAUNCH("gpt_resolve");
    return GPF_OK;
}

}  // extern "C"
