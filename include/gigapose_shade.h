/*
 * gigapose_shade.h -- C-ABI of libgigapose_shade.so: LIT renders of an untextured mesh on MI355X (gfx950), beside
 * libgigapose_render.so, whose gpr_project / gpr_raster write the keys this library reads (as libgigapose_texture.so does).
 * gpr_resolve draws "one white ambient light": a CAD model without colour or texture becomes a silhouette of one RGB value.
 * Reference: the reference renders exactly those datasets (T-LESS, ITODD: src/scripts/render_bop_templates.py:124) with
 * src/lib3d/blenderproc.py instead -- eight point lights around the camera (:27-37), a uniform grey of 0.4 (:46-49) -- so that
 * the lighting gives the template its interior signal.  This library is that lighting as a DIFFUSE model: smooth or flat
 * normals, Lambert's cosine, inverse-square fall-off, point lights given in camera coordinates, two host tables for the
 * transfer curves.  What of Blender's render it does not model (the specular lobe, path tracing, the view transform) is
 * listed in DESIGN.md; the contract is this header.  This library links no object of the other libraries.
 *
 * Conventions, return codes (0 = ok, -1 = invalid argument, -2 = launch failure) and gpl_last_error() are those of
 * gigapose_render.h: every pointer is a DEVICE pointer unless its name ends in _host, the caller owns all buffers, inputs are
 * never modified, `stream` is a hipStream_t passed as void*, calls are asynchronous.  Poses, K and pixel centres as there.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/shade_ref.py restates it in numpy and must agree bit for bit).  All
 * floating-point work is IEEE float64, one rounding per written operation, in the written order, no contraction (the library
 * is built with -ffp-contract=off) -- with ONE exception: root(x), the CORRECTLY ROUNDED square root that gigapose_dist.h
 * defines (the compiler's root, its two neighbours, two explicit fused multiply-adds that decide between them): what
 * numpy.sqrt returns.  The device evaluates no transcendental function.  Sums over faces are INTEGER sums, so no bit of a
 * vertex normal depends on the order of the faces, of a face's vertices, or of the threads.
 */
#ifndef GIGAPOSE_SHADE_H
#define GIGAPOSE_SHADE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpl_abi_version(void);
const char* gpl_last_error(void);

/* flags of gpl_vertex_normals, per vertex */
#define GPL_RANGE 1     /* a face at this vertex has a quantised cross product beyond 2^40, or one that is a NaN */
#define GPL_NO_NORMAL 2 /* the normal written is 0, 0, 0: no face, faces that cancel, or GPL_RANGE */
/* mode of gpl_shade */
#define GPL_SMOOTH 0
#define GPL_FLAT 1
#define GPL_MAX_LIGHTS 16

/* vertices (V,3) f32, faces (F,3) int32 -> acc (V,3) int64, flags (V) int32, normals (V,3) f64: smooth vertex normals, each
 * face weighted by its area.  The call initialises acc and flags (to 0) itself; two launches.
 * Per face with vertices i0, i1, i2 in the stored order, p_k = the float64 conversion of vertices[i_k]:
 *     u = p1 - p0,  v = p2 - p0        c = (u1*v2 - u2*v1,  u2*v0 - u0*v2,  u0*v1 - u1*v0)        [gpf_face_normals' c]
 *     q_k = rint(c_k * unit)            half to even; unit is a power of two, so the product is exact short of overflow
 *   - an index outside [0, V): the face is skipped (it flags nothing: it names no vertex);
 *   - every |q_k| <= 2^40 (false for a NaN): acc[i0], acc[i1], acc[i2] += q, 64-bit integer atomic adds (a vertex a face
 *     names twice is added to twice);
 *   - otherwise flags[i0], flags[i1], flags[i2] |= GPL_RANGE and nothing is added.
 * (c is twice the face's area times its unit normal and does not depend on which vertex comes first; rint is odd, so the
 * other winding gives exactly -q.)  Bound: at most 2^22 faces at one vertex -- 2^22 * 2^40 = 2^62 fits the accumulator.
 * Per vertex:
 *     a = (double)acc                   one rounding (|acc| can pass 2^53)
 *     aa = (ax*ax + ay*ay) + az*az
 *     n_k = a_k / root(aa)
 *   - aa == 0 or flags != 0: n = 0, 0, 0 and flags |= GPL_NO_NORMAL.
 * V >= 1, F >= 0; unit finite and > 0.  acc and normals 8-byte aligned. */
int gpl_vertex_normals(const float* vertices, int V, const int* faces, int F, double unit, long long* acc, int* flags, double* normals,
                       void* stream);

/* vis (N,H,W) u64, xy (N,V,2) int32, depth (N,V) f32, faces (F,3) int32, colours (V,3) u8 exactly as gpr_resolve takes them;
 * vertices (V,3) f32 (read in GPL_FLAT only; may be NULL otherwise), normals (V,3) f64 (read in GPL_SMOOTH only; may be NULL
 * otherwise; from gpl_vertex_normals or from the model file; need not be unit vectors), poses (N,4,4) f32 of which rows 0..2,
 * columns 0..2 are read, K_host[9] floats as gpr_project takes them, lights_host (L,4) f64 on the HOST: x, y, z in CAMERA
 * coordinates and model units, then the intensity I; 0 <= L <= GPL_MAX_LIGHTS (they travel in the kernel's arguments),
 * ambient f64, decode (256) f64: colour byte -> linear albedo, encode (T) u8: linear value -> output byte, 256 <= T <= 65536,
 * mode GPL_SMOOTH | GPL_FLAT  ->  rgba (N,H,W,4) u8, zdepth (N,H,W) f32 as gpr_resolve writes it, unlit (N) int32: the
 * number of covered pixels of the view without a usable normal; the call initialises it.  One thread per pixel.
 * Uncovered pixel (key all ones, or a face / vertex index out of range, a bad vertex, a face of no area): 0, 0, 0, 0 and depth
 * 0, as in gpr_resolve.  Covered pixel (px, py), face f = low 32 bits of the key:
 *   e_i, r_i as in gpr_raster (same swap),  t_i = e_i*r_i,  q = (t0 + t1) + t2
 *   c_ch = min(255, floor(((t0*c0 + t1*c1) + t2*c2) / q + 0.5)), not below 0      the byte gpr_resolve writes, per channel
 *   normal in model space
 *     GPL_SMOOTH   g_k = (t0*n0_k + t1*n1_k) + t2*n2_k     n_i = normals of vertex i AFTER the swap; no division by q: q > 0
 *                                                          and only the direction of g is used
 *     GPL_FLAT     g = c of gpl_vertex_normals above, from the face's STORED vertex order
 *   normal in camera space, P = the float64 conversion of poses[n]
 *     m_r = (P_r0*g0 + P_r1*g1) + P_r2*g2
 *   position, K = the float64 conversion of K_host
 *     z = (double) the f32 in the key's high 32 bits
 *     yn = (py - K5) / K4        xn = ((px - K2) - K1*yn) / K0        p = (xn*z, yn*z, z)
 *   the two-sided rule (both windings are drawn, so both are lit)
 *     s = (m0*p0 + m1*p1) + m2*p2;   s > 0: m = -m
 *   mm = (m0*m0 + m1*m1) + m2*m2;   !(mm > 0) or mm not below +inf: no light contributes and unlit[n] += 1
 *   irradiance
 *     E = ambient;  then for l = 0 .. L-1 in this order, when the normal is usable:
 *       d = light_l - p      dd = (d0*d0 + d1*d1) + d2*d2      md = (m0*d0 + m1*d1) + m2*d2
 *       md > 0 and dd > 0:   E = E + (I_l * md) / (root(mm * dd) * dd)         Lambert's cosine, inverse-square fall-off
 *   channel
 *     x = decode[c_ch] * E      i = floor(x * (T-1) + 0.5) clamped to [0, T-1], 0 for a NaN      byte = encode[i]
 *   alpha = 255, zdepth = the f32 of the key.
 * N <= 65535, H*W < 2^31; K_host[0] and K_host[4] must not be 0.  rgba 4-byte aligned (one pixel is written as one word),
 * normals and decode 8-byte aligned. */
int gpl_shade(const unsigned long long* vis, const int* xy, const float* depth, int V, const int* faces, int F, const uint8_t* colours,
              const float* vertices, const double* normals, const float* poses, const float* K_host, const double* lights_host, int L,
              double ambient, const double* decode, const uint8_t* encode, int T, int mode, int N, int H, int W, uint8_t* rgba,
              float* zdepth, int* unlit, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_SHADE_H */
