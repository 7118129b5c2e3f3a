// libgigapose_render.so (C-ABI: include/gigapose_render.h): the RGBA renders and depth maps of a vertex-coloured triangle mesh
// at N object poses, by a compute rasteriser -- an Instinct accelerator has no graphics pipeline.
//   reference: src/custom_megapose/call_panda3d.py:45-95 (Panda3D, one white ambient light, alpha = mask * 255, depth per view)
// gpr_project: one thread per (view, vertex).  gpr_raster: a z-buffer of 64-bit keys (depth bits << 32 | face) merged with
// atomicMin, so the image does not depend on the order of the triangles; one thread per (view, triangle) walks a small
// bounding box, a triangle with a large box goes to a list and a second launch gives it a whole workgroup.  gpr_resolve: one
// thread per pixel turns the key into colour, alpha and depth.  The arithmetic (int64 edge functions, float64 interpolation in
// a fixed order) is spelled out in the header and restated in gigapose_testing/raster_ref.py; the two agree bit for bit.
// The host-side plumbing is gp_front.h's; the triangle set-up, the coverage rule, what a resolve kernel reads out of a pixel's
// key and the vertex-colour byte are gp_raster_geom.h's (shared with the texture and shade libraries).  This library links no
// object of the other libraries and exports only gpr_* names.
#include <limits.h>
#include <math.h>

#include "gigapose_render.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpr
#include "../gp_front.h"
#include "../gp_raster_geom.h"   // Tri, setup_triangle, edges; Pixel, resolve_pixel, vertex_colour_byte

namespace {

constexpr int kThreads = 256;
constexpr double kMaxPixel = 16384.0;
constexpr int kSmallPixels = 288;        // bounding boxes of more pixels go to the workgroup-per-triangle launch (not measured: a few
                                         // rows of a wave's width; 287, 288 and 289 all factor into boxes a 64 x 48 test frame holds)
constexpr int kLargeBlocks = 2048;       // that launch: 8 workgroups on each of 256 CUs, striding the list
constexpr size_t kListHeader = 16;       // bytes in front of the list: the entry counter (u64) and padding

struct Cam {
    double k0, k1, k2, k3, k4, k5;
};

// grid (ceil(V / 256), N)
__global__ __launch_bounds__(kThreads) void project_kernel(const float* __restrict__ vertices, int V, const float* __restrict__ poses,
                                                           Cam K, float znear, int* __restrict__ xy, float* __restrict__ depth)
{
    const int v = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.y;
    if (v >= V) return;
    const float* P = poses + 16 * (size_t)n;
    const double x = vertices[3 * (size_t)v + 0], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    const double X = (((double)P[0] * x + (double)P[1] * y) + (double)P[2] * z) + (double)P[3];
    const double Y = (((double)P[4] * x + (double)P[5] * y) + (double)P[6] * z) + (double)P[7];
    const double Z = (((double)P[8] * x + (double)P[9] * y) + (double)P[10] * z) + (double)P[11];
    const double u = ((K.k0 * X + K.k1 * Y) + K.k2 * Z) / Z;
    const double w = ((K.k3 * X + K.k4 * Y) + K.k5 * Z) / Z;
    const float d = (float)Z;
    const bool good = d >= znear && fabs(u) <= kMaxPixel && fabs(w) <= kMaxPixel;   // false for every NaN
    const size_t o = (size_t)n * V + v;
    xy[2 * o + 0] = good ? (int)rint(u * 256.0) : kBadCoord;
    xy[2 * o + 1] = good ? (int)rint(w * 256.0) : kBadCoord;
    depth[o] = d;
}

__device__ __forceinline__ void sample(const Tri& t, int px, int py, unsigned f, u64* __restrict__ vis_n, int W)
{
    i64 e0, e1, e2;
    if (!edges(t, px, py, e0, e1, e2)) return;
    const double q = ((double)e0 * t.r0 + (double)e1 * t.r1) + (double)e2 * t.r2;
    const float z = (float)((double)t.area / q);
    atomicMin(vis_n + (size_t)py * W + px, (u64)__float_as_uint(z) << 32 | f);   // the value is not used: no return
}

// grid (ceil(F / 256), N): thread = (view, face).  A small box is walked here, row by row; a large one is listed.
__global__ __launch_bounds__(kThreads) void raster_small_kernel(const int* __restrict__ xy, const float* __restrict__ depth, int V,
                                                                const int* __restrict__ faces, int F, int H, int W,
                                                                u64* __restrict__ vis, int* __restrict__ clipped,
                                                                u64* __restrict__ count, u64* __restrict__ list)
{
    const int f = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.y;
    if (f >= F) return;
    Tri t;
    const int rc = setup_triangle(xy + 2 * (size_t)n * V, depth + (size_t)n * V, V, faces, f, H, W, true, t);
    if (rc == TRI_CLIPPED) atomicAdd(clipped + n, 1);
    if (rc != TRI_OK || t.bx1 < t.bx0 || t.by1 < t.by0) return;
    const i64 pixels = (i64)(t.bx1 - t.bx0 + 1) * (t.by1 - t.by0 + 1);
    if (pixels > kSmallPixels) {
        const u64 slot = atomicAdd(count, 1ull);   // < N * F: the list has one slot per (view, face)
        list[slot] = (u64)n << 32 | (unsigned)f;
        return;
    }
    u64* vis_n = vis + (size_t)n * H * W;
    for (int py = t.by0; py <= t.by1; ++py)
        for (int px = t.bx0; px <= t.bx1; ++px) sample(t, px, py, (unsigned)f, vis_n, W);
}

// grid (kLargeBlocks): a workgroup takes list entries blockIdx.x, + gridDim.x, ...; its threads stride the box, x fastest
__global__ __launch_bounds__(kThreads) void raster_large_kernel(const int* __restrict__ xy, const float* __restrict__ depth, int V,
                                                                const int* __restrict__ faces, int F, int N, int H, int W,
                                                                u64* __restrict__ vis, const u64* __restrict__ count,
                                                                const u64* __restrict__ list)
{
    const u64 total = min(*count, (u64)N * (u64)F);
    for (u64 i = blockIdx.x; i < total; i += gridDim.x) {
        const u64 entry = list[i];
        const int n = (int)(entry >> 32), f = (int)(entry & 0xffffffffu);
        if (n >= N || f >= F) continue;   // uniform over the workgroup
        Tri t;
        if (setup_triangle(xy + 2 * (size_t)n * V, depth + (size_t)n * V, V, faces, f, H, W, true, t) != TRI_OK) continue;
        const int bw = t.bx1 - t.bx0 + 1, bh = t.by1 - t.by0 + 1;
        if (bw <= 0 || bh <= 0) continue;
        u64* vis_n = vis + (size_t)n * H * W;
        const unsigned pixels = (unsigned)bw * (unsigned)bh;   // <= H*W < 2^31
        int row = threadIdx.x / bw, col = threadIdx.x - row * bw;
        const int step_r = kThreads / bw, step_c = kThreads % bw;
        for (unsigned p = threadIdx.x; p < pixels; p += kThreads) {
            sample(t, t.bx0 + col, t.by0 + row, (unsigned)f, vis_n, W);
            row += step_r;
            col += step_c;
            if (col >= bw) {
                col -= bw;
                ++row;
            }
        }
    }
}

// grid (ceil(H*W / 256), N): thread = pixel
__global__ __launch_bounds__(kThreads) void resolve_kernel(const u64* __restrict__ vis, const int* __restrict__ xy,
                                                           const float* __restrict__ depth, int V, const int* __restrict__ faces, int F,
                                                           const uint8_t* __restrict__ colours, int H, int W,
                                                           uint32_t* __restrict__ rgba, float* __restrict__ zdepth)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (p >= (unsigned)H * (unsigned)W) return;
    const size_t o = (size_t)n * H * W + p;
    uint32_t px = 0u;
    Pixel pixel;
    resolve_pixel(vis[o], p, xy + 2 * (size_t)n * V, depth + (size_t)n * V, V, faces, F, H, W, pixel, [&](const Pixel& pix) {
        px = 0xff000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) px |= vertex_colour_byte(colours, pix, c) << (8 * c);
    });
    rgba[o] = px;
    zdepth[o] = pixel.z;
}

}  // namespace

extern "C" {

int gpr_abi_version(void) { return 1; }
int gpr_small_triangle_pixels(void) { return kSmallPixels; }

size_t gpr_raster_workspace_bytes(int N, int F)
{
    if (N < 0 || F < 0) return 0;
    return kListHeader + (size_t)N * (size_t)F * sizeof(u64);
}

int gpr_project(const float* vertices, int V, const float* poses, int N, const float* K_host, float znear, int* xy, float* depth,
                void* stream)
{
    GPF_REQUIRE(V >= 0 && N >= 0 && N <= 65535, "gpr_project: bad sizes (V >= 0, 0 <= N <= 65535)");
    GPF_REQUIRE(znear >= 1e-30f && znear <= 3.0e38f, "gpr_project: znear must be finite and >= 1e-30");
    if (N == 0 || V == 0) return GPF_OK;
    GPF_REQUIRE(vertices && poses && K_host && xy && depth, "gpr_project: null pointer");
    GPF_REQUIRE(K_host[6] == 0.0f && K_host[7] == 0.0f && K_host[8] == 1.0f, "gpr_project: the last row of K must be 0, 0, 1");
    const Cam K = {K_host[0], K_host[1], K_host[2], K_host[3], K_host[4], K_host[5]};
    hipLaunchKernelGGL(project_kernel, dim3((V + kThreads - 1) / kThreads, N), dim3(kThreads), 0, (hipStream_t)stream, vertices, V,
                       poses, K, znear, xy, depth);
    GPF_CHECK_LAUNCH("gpr_project");
    return GPF_OK;
}

int gpr_raster(const int* xy, const float* depth, int V, const int* faces, int F, int N, int H, int W, unsigned long long* vis,
               int* clipped, void* workspace, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W) && V >= 0 && F >= 0, "gpr_raster: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31, V, F >= 0)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && clipped, "gpr_raster: null pointer");
    GPF_REQUIRE(((uintptr_t)vis & 7) == 0, "gpr_raster: vis is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    if (F > 0) {   // checked before anything is enqueued
        GPF_REQUIRE(xy && depth && faces && workspace, "gpr_raster: null pointer");
        GPF_REQUIRE(((uintptr_t)workspace & 7) == 0, "gpr_raster: workspace is not 8-byte aligned");
    }
    GPF_CHECK_HIP("gpr_raster", hipMemsetAsync(vis, 0xff, (size_t)N * H * W * sizeof(u64), s));
    GPF_CHECK_HIP("gpr_raster", hipMemsetAsync(clipped, 0, (size_t)N * sizeof(int), s));
    if (F == 0) return GPF_OK;
    u64* count = reinterpret_cast<u64*>(workspace);
    u64* list = reinterpret_cast<u64*>(reinterpret_cast<char*>(workspace) + kListHeader);
    GPF_CHECK_HIP("gpr_raster", hipMemsetAsync(workspace, 0, kListHeader, s));
    hipLaunchKernelGGL(raster_small_kernel, dim3((F + kThreads - 1) / kThreads, N), dim3(kThreads), 0, s, xy, depth, V, faces, F, H, W,
                       vis, clipped, count, list);
    GPF_CHECK_LAUNCH("gpr_raster");
    const u64 slots = (u64)N * (u64)F;
    const int blocks = slots < (u64)kLargeBlocks ? (int)slots : kLargeBlocks;
    hipLaunchKernelGGL(raster_large_kernel, dim3(blocks), dim3(kThreads), 0, s, xy, depth, V, faces, F, N, H, W, vis, count, list);
    GPF_CHECK_LAUNCH("gpr_raster");
    return GPF_OK;
}

int gpr_resolve(const unsigned long long* vis, const int* xy, const float* depth, int V, const int* faces, int F,
                const uint8_t* colours, int N, int H, int W, uint8_t* rgba, float* zdepth, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W) && V >= 0 && F >= 0, "gpr_resolve: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31, V, F >= 0)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && rgba && zdepth, "gpr_resolve: null pointer");
    GPF_REQUIRE(F == 0 || (xy && depth && faces && colours), "gpr_resolve: null pointer");
    GPF_REQUIRE(((uintptr_t)rgba & 3) == 0, "gpr_resolve: rgba is not 4-byte aligned (one pixel is one word)");
    const unsigned blocks = (unsigned)(((long long)H * W + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks, N), dim3(kThreads), 0, (hipStream_t)stream, vis, xy, depth, V, faces, F, colours, H,
                       W, reinterpret_cast<uint32_t*>(rgba), zdepth);
    GPF_CHECK_LAUNCH("gpr_resolve");
    return GPF_OK;
}

}  // extern "C"
