// The triangle arithmetic of the compute rasteriser, shared by render/gpr_render.hip (raster + coloured resolve) and
// texture/gpt_texture.hip (textured resolve).  Header only; written ONCE: the two libraries must never disagree on which
// pixels a triangle owns, on the 1 <-> 2 vertex swap of a negative area, or on r_i = 1.0 / (double)depth_i.  The arithmetic is
// spelled out in include/gigapose_render.h (gpr_raster) and restated in gigapose_testing/raster_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kBadCoord = INT_MIN;

// One triangle of one view, set up: vertices ordered so that area > 0, the pixel box clamped to the frame.
struct Tri {
    i64 x0, y0, x1, y1, x2, y2, area;
    double r0, r1, r2;
    int i0, i1, i2;           // the vertex indices in the order used (1 and 2 swapped when the winding was negative)
    int bx0, by0, bx1, by1;   // inclusive pixel box; empty when bx1 < bx0 or by1 < by0
    bool swapped;             // the winding was negative: corner k of the face is now corner (0, 2, 1)[k]; whatever the caller
                              // keeps per corner (texture coordinates) has to be swapped with the vertices
};

enum { TRI_OK = 0, TRI_CLIPPED = 1, TRI_SKIP = 2 };

__device__ __forceinline__ i64 imin3(i64 a, i64 b, i64 c) { return min(a, min(b, c)); }
__device__ __forceinline__ i64 imax3(i64 a, i64 b, i64 c) { return max(a, max(b, c)); }

// `box` = false leaves the pixel box unset (the resolve kernels do not need it)
__device__ __forceinline__ int setup_triangle(const int* __restrict__ xy_n, const float* __restrict__ depth_n, int V,
                                              const int* __restrict__ faces, int f, int H, int W, bool box, Tri& t)
{
    const int i0 = faces[3 * (size_t)f + 0];
    int i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return TRI_CLIPPED;
    t.x0 = xy_n[2 * (size_t)i0];
    t.x1 = xy_n[2 * (size_t)i1];
    t.x2 = xy_n[2 * (size_t)i2];
    if (t.x0 == kBadCoord || t.x1 == kBadCoord || t.x2 == kBadCoord) return TRI_CLIPPED;
    t.y0 = xy_n[2 * (size_t)i0 + 1];
    t.y1 = xy_n[2 * (size_t)i1 + 1];
    t.y2 = xy_n[2 * (size_t)i2 + 1];
    t.area = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
    if (t.area == 0) return TRI_SKIP;
    t.swapped = t.area < 0;
    if (t.swapped) {
        i64 s = t.x1; t.x1 = t.x2; t.x2 = s;
        s = t.y1; t.y1 = t.y2; t.y2 = s;
        const int k = i1; i1 = i2; i2 = k;
        t.area = -t.area;
    }
    t.i0 = i0;
    t.i1 = i1;
    t.i2 = i2;
    t.r0 = 1.0 / (double)depth_n[i0];
    t.r1 = 1.0 / (double)depth_n[i1];
    t.r2 = 1.0 / (double)depth_n[i2];
    if (box) {
        // ceil(min / 256) and floor(max / 256) by arithmetic shifts, clamped to the frame
        const i64 lx = (imin3(t.x0, t.x1, t.x2) + 255) >> 8, hx = imax3(t.x0, t.x1, t.x2) >> 8;
        const i64 ly = (imin3(t.y0, t.y1, t.y2) + 255) >> 8, hy = imax3(t.y0, t.y1, t.y2) >> 8;
        t.bx0 = (int)max(lx, (i64)0);
        t.bx1 = (int)min(hx, (i64)W - 1);
        t.by0 = (int)max(ly, (i64)0);
        t.by1 = (int)min(hy, (i64)H - 1);
    }
    return TRI_OK;
}

__device__ __forceinline__ bool edge_in(i64 e, i64 dx, i64 dy) { return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0))); }

// edge values of pixel (px, py); returns whether the pixel is inside
__device__ __forceinline__ bool edges(const Tri& t, int px, int py, i64& e0, i64& e1, i64& e2)
{
    const i64 X = (i64)px * 256, Y = (i64)py * 256;
    const i64 dx0 = t.x2 - t.x1, dy0 = t.y2 - t.y1;   // edge 1 -> 2
    const i64 dx1 = t.x0 - t.x2, dy1 = t.y0 - t.y2;   // edge 2 -> 0
    const i64 dx2 = t.x1 - t.x0, dy2 = t.y1 - t.y0;   // edge 0 -> 1
    e0 = dx0 * (Y - t.y1) - dy0 * (X - t.x1);
    e1 = dx1 * (Y - t.y2) - dy1 * (X - t.x2);
    e2 = dx2 * (Y - t.y0) - dy2 * (X - t.x0);
    return edge_in(e0, dx0, dy0) && edge_in(e1, dx1, dy1) && edge_in(e2, dx2, dy2);
}

}  // namespace
