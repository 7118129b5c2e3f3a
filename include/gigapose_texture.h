/*
 * gigapose_texture.h -- C-ABI of libgigapose_texture.so: textured template rendering on MI355X (gfx950).  The library stands
 * beside libgigapose_render.so: gpr_project and gpr_raster draw the visibility keys of a mesh, gpt_resolve turns them into
 * the RGBA renders and depth maps with the colour taken from ONE texture image through per-corner UV coordinates, filtered
 * trilinearly over a mip pyramid that gpt_build_mips makes.  Reference: the Panda3D render of
 * src/custom_megapose/call_panda3d.py:45-95 with the texture filters of
 * src/megapose/panda3d_renderer/panda3d_scene_renderer.py:70-71 (mip-mapped minification, repeat wrapping, one white ambient
 * light: the colour is the texel, unshaded).  This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_render.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpt_last_error() returns a thread-local message
 *     for the last failure; arguments are checked before anything is enqueued; N = 0 is a successful no-op.
 *
 * Limits: 1 <= Ht, Wt <= GPT_MAX_TEXTURE; N <= 65535 per call, H*W < 2^31, F < 2^31, V < 2^31; every buffer is addressed
 * through size_t.
 *
 * Out of scope: anisotropic filtering, several textures per model, vertex colour x texture modulation, and as in
 * gigapose_render.h near-plane clipping, shading and anti-aliasing.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/texture_ref.py restates it in numpy and must agree bit for bit).
 * All floating-point work is IEEE float64, one rounding per written operation, in the written order, no fused
 * multiply-add (-ffp-contract=off); only + - * /, floor and comparisons are used -- no sqrt, log2 or exp2, whose last bit
 * is not guaranteed to agree between numpy and the device.  Division is the correctly rounded one (see gigapose_render.h).
 */
#ifndef GIGAPOSE_TEXTURE_H
#define GIGAPOSE_TEXTURE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpt_abi_version(void);
const char* gpt_last_error(void);

#define GPT_MAX_TEXTURE 16384 /* the largest texture height / width */
#define GPT_MAX_UV 32768.0f   /* a corner UV beyond this in magnitude (or not finite) makes its face's UV bad; see gpt_resolve */

/* THE PYRAMID.  Level 0 is the image, Ht rows of Wt texels, row 0 = the TOP row (as PIL reads it).  Level l+1 has
 * H_{l+1} = max(1, H_l >> 1) rows and W_{l+1} = max(1, W_l >> 1) columns, down to 1 x 1: gpt_mip_levels = 1 + floor(log2(max(Ht,
 * Wt))) levels.  The levels are packed one after another, level 0 first, each row-major: gpt_mip_texels = sum of H_l * W_l.
 * Both return 0 when Ht or Wt is outside [1, GPT_MAX_TEXTURE]. */
int gpt_mip_levels(int Ht, int Wt);
size_t gpt_mip_texels(int Ht, int Wt);

/* rgb (Ht,Wt,3) u8 -> pyramid, gpt_mip_texels(Ht, Wt) 32-bit words.  A texel is one word R | G << 8 | B << 16 | 0xff << 24
 * (the pixel format of the renders).  Texel (row i, column j) of level l+1 is, per channel (the alpha byte included: it stays
 * 0xff), (a + b + c + d + 2) >> 2 of the texels (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1) of level l, every source index
 * clamped to its size - 1: an odd last row or column is dropped, and the clamp matters only once a dimension has reached 1.
 * pyramid must be 4-byte aligned.  One launch per level; every word of the pyramid is written. */
int gpt_build_mips(const uint8_t* rgb, int Ht, int Wt, uint32_t* pyramid, void* stream);

/* vis (N,H,W) u64, xy (N,V,2) int32, depth (N,V) f32, faces (F,3) int32 as gpr_project / gpr_raster write them; corner_uv
 * (F,3,2) f32: (u, v) of corner k of face f -- per CORNER, so that two faces may give a shared vertex different UVs (seams);
 * pyramid as gpt_build_mips writes it for an Ht x Wt image -> rgba (N,H,W,4) u8, zdepth (N,H,W) f32.  One thread per pixel.
 *
 * Uncovered pixel (gpr_resolve's rule: key all ones, a face index >= F, a vertex index outside [0, V), a bad vertex, area 0):
 * 0, 0, 0, 0 and depth 0.  Covered pixel: alpha = 255, zdepth = the f32 whose bits are the high 32 bits of the key, and the
 * colour as follows.  Face = low 32 bits of the key; e_i, r_i as in gpr_raster, after the same 1 <-> 2 swap on negative area,
 * and (u_i, v_i) = the UV of corner i AFTER that swap (corner_uv[f][(0, 2, 1)[i]] when swapped), converted to float64.
 *
 *   UV at a sample with edge values e_i:  t_i = (double)e_i * r_i;  q = (t0 + t1) + t2;
 *       u = ((t0*u0 + t1*u1) + t2*u2) / q;   v = ((t0*v0 + t1*v1) + t2*v2) / q            (perspective-correct)
 *   It is evaluated at the pixel (x, y) -> q, u, v; at (x+1, y) with the exact int64 e_i - 256*dy_i -> qx, ux, vx; and at
 *   (x, y+1) with e_i + 256*dx_i -> qy, uy, vy, where (dx_i, dy_i) is the direction of edge i (gpr_raster).  The neighbours are
 *   the SAME triangle's interpolant, whether or not the triangle covers them.
 *
 *   Bad UV: any of the face's six corner values c fails -GPT_MAX_UV <= c <= GPT_MAX_UV, or the pixel's u or v fails
 *   -2*GPT_MAX_UV <= . <= 2*GPT_MAX_UV (every comparison is false for a NaN).  The pixel is 0, 0, 0 with alpha 255 and its
 *   depth.  [The corner test makes a bad corner blacken exactly the pixels of its face; the pixel test bounds every texel
 *   index whatever the depths are: |u * W_l| <= 2^16 * 2^14 = 2^30, so floor() fits an int32 and s - floor(s) is exact.]
 *
 *   Level of detail, L = gpt_mip_levels(Ht, Wt), top = L - 1:
 *     1. qx <= 0 or qy <= 0 (false for a NaN): level top alone (the plane's horizon lies within one pixel).
 *     2. dsdx = (ux - u) * Wt;  dtdx = (vx - v) * Ht;  dsdy = (uy - u) * Wt;  dtdy = (vy - v) * Ht;
 *        ax = dsdx*dsdx + dtdx*dtdx;  ay = dsdy*dsdy + dtdy*dtdy;  ax or ay is a NaN: level top alone.
 *        rho2 = ay > ax ? ay : ax.
 *     3. rho2 < 1: level 0 alone (magnification).
 *     4. l0 = the largest level <= top with 4^l0 <= rho2 (exact comparisons with powers of two).  l0 == top: level top alone.
 *        Otherwise levels l0 and l0 + 1 are blended with  w = (rho2 / 4^l0 - 1) / 3  in [0, 1).
 *        [The textbook level is log2(rho) = log2(rho2) / 2 and the weight its fraction.  w is a monotone blend in rho SQUARED
 *        that stands in for the fractional logarithm: it is 0 at rho2 = 4^l0 and reaches 1 at 4^(l0+1), so the result is
 *        continuous across levels, and it needs no transcendental.  With x = rho2 / 4^l0 the logarithm's fraction is
 *        log2(x) / 2; w lies below it by at most 0.17 (at x = 2.16): the blend is that much sharper in mid-level.]
 *
 *   Bilinear sample of level l (H_l rows, W_l columns), per channel c of the texels:
 *     s = u * W_l - 0.5;  t = (1 - v) * H_l - 0.5      (UV origin bottom-left as in PLY / OBJ files; image row 0 on top)
 *     i0 = floor(s);  fx = s - i0;  j0 = floor(t);  fy = t - j0
 *     columns i0 and i0 + 1 taken modulo W_l, rows j0 and j0 + 1 modulo H_l (mathematical modulo: repeat wrapping)
 *     A = ((1-fx)*c00 + fx*c10) * (1-fy) + ((1-fx)*c01 + fx*c11) * fy        c_ab = column i0 + a, row j0 + b
 *   Output channel: one level alone: min(255, floor(A + 0.5)); two levels (A from l0, B from l0 + 1):
 *     min(255, floor(((1-w)*A + w*B) + 0.5)).
 * rgba must be 4-byte aligned (one pixel is written as one word), pyramid likewise. */
int gpt_resolve(const unsigned long long* vis, const int* xy, const float* depth, int V, const int* faces, int F,
                const float* corner_uv, const uint32_t* pyramid, int Ht, int Wt, int N, int H, int W, uint8_t* rgba, float* zdepth,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_TEXTURE_H */
