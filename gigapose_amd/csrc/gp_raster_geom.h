// The triangle and pixel arithmetic of the compute rasteriser, shared by render/gpr_render.hip (raster + coloured resolve),
// texture/gpt_texture.hip (textured resolve) and shade/gpl_shade.hip (lit resolve).  Header only; written ONCE: the three
// libraries must never disagree on which pixels a triangle owns, on the 1 <-> 2 vertex swap of a negative area, on
// r_i = 1.0 / (double)depth_i, or -- in the resolve kernels -- on which keys are background, on the weights t_k = e_k * r_k
// and their sum q, on the depth a key carries and on how a float64 colour becomes a byte.  The arithmetic is spelled out in
// include/gigapose_render.h (gpr_raster, gpr_resolve) and restated in gigapose_testing/raster_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
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

// One pixel of a resolve kernel: what its key says, before any colour.
struct Pixel {
    Tri t;                 // the face the key names, set up in this view (no pixel box)
    i64 e0, e1, e2;        // the edge values at the pixel's centre
    double t0, t1, t2, q;  // t_k = (double)e_k * t.r_k, q = (t0 + t1) + t2: perspective-correct weights are t_k / q
    int x, y;
    unsigned f;            // the key's lower word
    float z;               // the key's upper word as a float; 0 when the pixel is not drawn
};

// The key of pixel p (row-major in the H x W frame of a view whose projected vertices are xy_n, depth_n) -> whether the pixel is
// drawn: the key is not the empty one, names a face < F and that face sets up.  Nothing but f and z is set otherwise.  A drawn
// pixel is handed to colour(s) -- the kernel's own part, a lambda -- HERE and not after the return: code that follows a returned bool is
// compiled as a region of its own, whose loads (colours, UVs, normals) wait for the set-up's depth loads instead of going
// out beside them; that round trip to memory cost the three resolve kernels 2 to 5%.
template <class Colour>
__device__ __forceinline__ bool resolve_pixel(u64 key, unsigned p, const int* __restrict__ xy_n, const float* __restrict__ depth_n,
                                              int V, const int* __restrict__ faces, int F, int H, int W, Pixel& s, Colour colour)
{
    s.f = (unsigned)(key & 0xffffffffu);
    s.z = 0.0f;
    if (key == ~0ull || s.f >= (unsigned)F || setup_triangle(xy_n, depth_n, V, faces, (int)s.f, H, W, false, s.t) != TRI_OK) return false;
    s.y = (int)(p / (unsigned)W);
    s.x = (int)(p - (unsigned)s.y * (unsigned)W);
    edges(s.t, s.x, s.y, s.e0, s.e1, s.e2);
    s.t0 = (double)s.e0 * s.t.r0, s.t1 = (double)s.e1 * s.t.r1, s.t2 = (double)s.e2 * s.t.r2;
    s.q = (s.t0 + s.t1) + s.t2;
    s.z = __uint_as_float((unsigned)(key >> 32));
    colour(s);
    return true;
}

// floor(x + 1/2) clamped to a byte; a NaN gives 0
__device__ __forceinline__ unsigned to_byte(double x)
{
    const double v = floor(x + 0.5);
    return v >= 255.0 ? 255u : (v > 0.0 ? (unsigned)v : 0u);
}

// channel c of the perspective-correct mix of the three vertex colours (u8 (V,3))
__device__ __forceinline__ unsigned vertex_colour_byte(const uint8_t* __restrict__ colours, const Pixel& s, int c)
{
    const double c0 = colours[3 * (size_t)s.t.i0 + c], c1 = colours[3 * (size_t)s.t.i1 + c], c2 = colours[3 * (size_t)s.t.i2 + c];
    return to_byte(((s.t0 * c0 + s.t1 * c1) + s.t2 * c2) / s.q);
}

}  // namespace
