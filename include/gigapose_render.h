/*
 * gigapose_render.h -- C-ABI of libgigapose_render.so: template rendering on MI355X (gfx950), the stage in front of
 * libgigapose_onboard.so.  A triangle mesh with per-vertex colours is drawn at N object poses by a compute rasteriser: a
 * z-buffer of 64-bit keys merged with an integer atomic minimum, then one pass that turns the keys into the RGBA renders
 * gpo_alpha_boxes / gpo_crop_templates read and a depth map beside each.  Reference: the Panda3D render of
 * src/custom_megapose/call_panda3d.py:45-95 -- one white ambient light (the colour is the albedo, unshaded), alpha = the
 * binary mask * 255, a depth map per view.  This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_onboard.h)
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all buffers, kernels never allocate;
 *     inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpr_last_error() returns a thread-local message
 *     for the last failure.
 *
 * Geometry: poses are object -> camera, row-major 4x4 f32, OpenCV convention (x right, y down, z forward): what the
 * reference's load_pose returns.  K is a HOST array of 9 floats, row-major, with K[6..8] = 0, 0, 1.  Pixel centres sit at
 * integer coordinates (BOP): pixel (px, py) is the sample point u = px, v = py.
 *
 * Limits: N <= 65535 per call (the grid's second dimension; gigapose_amd/render.py chunks the views), H*W < 2^31,
 * F < 2^31, V < 2^31; every buffer is addressed through size_t (one view of the visibility buffer is H*W*8 bytes, so the
 * buffer passes 2^31 bytes at 162 views of 480 x 640).
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/raster_ref.py restates it in numpy and must agree bit for bit).
 * All floating-point work is IEEE float64, one rounding per written operation, in the written order, no fused
 * multiply-add (the library is built with -ffp-contract=off).  Division: hipcc's default for gfx950 expands a float64 `/`
 * to the correctly rounded sequence (v_div_scale / v_div_fmas / v_div_fixup) unless -ffast-math or
 * -fno-hip-fp32-correctly-rounded-divide-sqrt style options say otherwise; -fhip-fp32-correctly-rounded-divide-sqrt (the
 * default, ON) does the same for float32.  The build passes neither -ffast-math nor the negative form, so no extra option
 * is needed; the kernels use float64 division only.
 */
#ifndef GIGAPOSE_RENDER_H
#define GIGAPOSE_RENDER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpr_abi_version(void);
const char* gpr_last_error(void);

/* Screen coordinates are int32 in units of 1/256 pixel.  A bad vertex has both coordinates = GPR_BAD_COORD. */
#define GPR_BAD_COORD (-2147483647 - 1)
#define GPR_MAX_PIXEL 16384 /* |u|, |v| beyond this many pixels make a vertex bad: coordinates stay below 2^23 */

/* vertices (V,3) f32, poses (N,4,4) f32 -> xy (N,V,2) int32, depth (N,V) f32.  With P = poses[n], (x,y,z) = vertices[v], all
 * converted to float64:
 *     X = ((P00*x + P01*y) + P02*z) + P03      Y, Z likewise from rows 1, 2
 *     u = ((K0*X + K1*Y) + K2*Z) / Z          v = ((K3*X + K4*Y) + K5*Z) / Z
 *     depth = (float)Z                          xy = (int)rint(u * 256), (int)rint(v * 256)     [rint: half to even]
 * The vertex is good iff depth >= znear and |u| <= GPR_MAX_PIXEL and |v| <= GPR_MAX_PIXEL (every comparison is false for a
 * NaN, so anything non-finite is bad).  A bad vertex gets xy = GPR_BAD_COORD, GPR_BAD_COORD; its depth is written as computed.
 * znear must be finite and >= 1e-30. */
int gpr_project(const float* vertices, int V, const float* poses, int N, const float* K_host, float znear, int* xy, float* depth,
                void* stream);

/* The pixel count of a triangle's bounding box (clamped to the frame) above which gpr_raster hands the triangle to the
 * one-workgroup-per-triangle launch; at or below it one thread walks the box. */
int gpr_small_triangle_pixels(void);
/* Bytes of the workspace gpr_raster needs for N views of F faces (a counter and one 8-byte entry per (view, face)). */
size_t gpr_raster_workspace_bytes(int N, int F);

/* xy (N,V,2), depth (N,V) as gpr_project writes them, faces (F,3) int32 -> vis (N,H,W) u64, clipped (N) int32.  The call
 * initialises vis (every key to all ones = uncovered), clipped (to 0) and the workspace itself.
 * Key of a covered sample: ((uint64)bits of the f32 depth << 32) | face index, merged per pixel with a 64-bit unsigned atomic
 * minimum: the nearest surface wins, on exactly equal depth the lower face index, whatever the order of arrival.
 * Per (view, face) with vertices 0, 1, 2 (all integer arithmetic in int64):
 *   - a vertex index outside [0, V) or a bad vertex: the triangle is dropped and clipped[n] += 1 (no near-plane clipping);
 *   - area = (x1-x0)*(y2-y0) - (y1-y0)*(x2-x0); area < 0: vertices 1 and 2 (and their depths) are swapped and area = -area
 *     (both windings are drawn, no back-face culling); area == 0: skipped;
 *   - bounding box: pixels px in [ceil(min x / 256), floor(max x / 256)] clamped to [0, W-1], py likewise;
 *   - pixel (i, j) is the point p = (256*i, 256*j); the edge value of edge a->b there is e = (bx-ax)*(py-ay) - (by-ay)*(px-ax);
 *     e0 belongs to edge 1->2, e1 to 2->0, e2 to 0->1 (e0 + e1 + e2 = area; e_i / area is vertex i's barycentric);
 *   - p is inside iff for every edge e > 0, or e == 0 and (dy < 0 or (dy == 0 and dx > 0)) with dx = bx-ax, dy = by-ay
 *     (the top-left rule: a shared edge is covered exactly once);
 *   - depth, perspective-correct: r_i = 1.0 / (double)depth_i;  q = (e0*r0 + e1*r1) + e2*r2;  z = (double)area / q;
 *     the key holds the bits of (float)z.
 * workspace: gpr_raster_workspace_bytes(N, F) bytes, 8-byte aligned. */
int gpr_raster(const int* xy, const float* depth, int V, const int* faces, int F, int N, int H, int W, unsigned long long* vis,
               int* clipped, void* workspace, void* stream);

/* vis, xy, depth, faces as above, colours (V,3) u8 -> rgba (N,H,W,4) u8 (the format of gigapose_onboard.h), zdepth (N,H,W) f32.
 * Uncovered pixel (key all ones, or a face / vertex index out of range): 0, 0, 0, 0 and depth 0.  Covered pixel: face = low
 * 32 bits of the key, e_i and r_i as in gpr_raster (same swap), t_i = e_i*r_i, q = (t0 + t1) + t2,
 *     channel c = min(255, floor(((t0*c0 + t1*c1) + t2*c2) / q + 0.5))      alpha = 255
 *     zdepth = the f32 whose bits are the high 32 bits of the key, in model units.
 * rgba must be 4-byte aligned (one pixel is written as one word). */
int gpr_resolve(const unsigned long long* vis, const int* xy, const float* depth, int V, const int* faces, int F,
                const uint8_t* colours, int N, int H, int W, uint8_t* rgba, float* zdepth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_RENDER_H */
