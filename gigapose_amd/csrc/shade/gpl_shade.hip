// libgigapose_shade.so (C-ABI: include/gigapose_shade.h): diffuse shading of an untextured mesh under point lights, beside
// libgigapose_render.so, whose gpr_project / gpr_raster write the keys this library reads.
//   reference: src/lib3d/blenderproc.py:27-49 (eight point lights around the camera, a uniform grey), the route of
//   src/scripts/render_bop_templates.py:124 for T-LESS and ITODD
// gpl_vertex_normals: one thread per face adds its quantised cross product to its three vertices with 64-bit integer atomics
// (an integer sum: the bits depend on no order), then one thread per vertex normalises.  gpl_shade: one thread per pixel; the
// colour byte of gpr_resolve, a normal (interpolated, or the face's), the camera-space position from the key's depth, and a
// loop over at most 16 lights that sit in the kernel's arguments: per light 3 subtractions, two dot products, one root and one
// division.  Background pixels leave after the key.  The arithmetic is spelled out in the header and restated in
// gigapose_testing/shade_ref.py; the two agree bit for bit.  The host-side plumbing is gp_front.h's; the triangle set-up,
// what the kernel reads out of a pixel's key (the gate, the weights, the depth) and the vertex-colour byte are gp_raster_geom.h's
// (shared with the render and texture libraries), the square root gp_root.h's (shared with the distance library).  This
// library links no object of the other libraries and exports only gpl_* names.
#include <math.h>

#include "gigapose_shade.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpl
#include "../gp_front.h"
#include "../gp_raster_geom.h"
#include "../gp_root.h"

namespace {

constexpr int kThreads = 256;
constexpr double kMaxQuantum = 0x1p40;
constexpr double kInf = (double)INFINITY;

// the face's cross product from its stored vertex order (gpf_face_normals' arithmetic); the indices are in range
__device__ __forceinline__ void face_cross(const float* __restrict__ vertices, int i0, int i1, int i2, double* c)
{
    const float *p0 = vertices + 3 * (size_t)i0, *p1 = vertices + 3 * (size_t)i1, *p2 = vertices + 3 * (size_t)i2;
    const double u0 = (double)p1[0] - (double)p0[0], u1 = (double)p1[1] - (double)p0[1], u2 = (double)p1[2] - (double)p0[2];
    const double v0 = (double)p2[0] - (double)p0[0], v1 = (double)p2[1] - (double)p0[1], v2 = (double)p2[2] - (double)p0[2];
    c[0] = u1 * v2 - u2 * v1, c[1] = u2 * v0 - u0 * v2, c[2] = u0 * v1 - u1 * v0;
}

// grid (ceil(F / 256)): thread = face.  acc, flags: zeroed by the caller
__global__ __launch_bounds__(kThreads) void accumulate_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces, int F,
                                                              double unit, unsigned long long* __restrict__ acc, int* __restrict__ flags)
{
    const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int idx[3] = {faces[3 * (size_t)f + 0], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
    if ((unsigned)idx[0] >= (unsigned)V || (unsigned)idx[1] >= (unsigned)V || (unsigned)idx[2] >= (unsigned)V) return;
    double c[3];
    face_cross(vertices, idx[0], idx[1], idx[2], c);
    const double q0 = rint(c[0] * unit), q1 = rint(c[1] * unit), q2 = rint(c[2] * unit);
    if (fabs(q0) <= kMaxQuantum && fabs(q1) <= kMaxQuantum && fabs(q2) <= kMaxQuantum) {   // false for a NaN
        const long long q[3] = {(long long)q0, (long long)q1, (long long)q2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            unsigned long long* a = acc + 3 * (size_t)idx[k];
#pragma unroll
            for (int j = 0; j < 3; ++j) atomicAdd(a + j, (unsigned long long)q[j]);   // two's complement: the signed sum
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicOr(flags + idx[k], GPL_RANGE);
    }
}

// grid (ceil(V / 256)): thread = vertex
__global__ __launch_bounds__(kThreads) void normalise_kernel(const long long* __restrict__ acc, int V, int* __restrict__ flags,
                                                             double* __restrict__ normals)
{
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const double ax = (double)acc[3 * (size_t)v + 0], ay = (double)acc[3 * (size_t)v + 1], az = (double)acc[3 * (size_t)v + 2];
    const double aa = (ax * ax + ay * ay) + az * az;
    const int fl = flags[v];
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (aa == 0.0 || fl != 0) {
        flags[v] = fl | GPL_NO_NORMAL;
    } else {
        const double r = root(aa);
        n0 = ax / r, n1 = ay / r, n2 = az / r;
    }
    normals[3 * (size_t)v + 0] = n0, normals[3 * (size_t)v + 1] = n1, normals[3 * (size_t)v + 2] = n2;
}

// what does not depend on the pixel, by value in the kernel's arguments
struct Scene {
    double K0, K1, K2, K4, K5;
    double ambient;
    double light[GPL_MAX_LIGHTS][4];
    int L;
};

// grid (ceil(H*W / 256), N): thread = pixel
template <bool kFlat>
__global__ __launch_bounds__(kThreads) void shade_kernel(const u64* __restrict__ vis, const int* __restrict__ xy,
                                                         const float* __restrict__ depth, int V, const int* __restrict__ faces, int F,
                                                         const uint8_t* __restrict__ colours, const float* __restrict__ vertices,
                                                         const double* __restrict__ normals, const float* __restrict__ poses, Scene S,
                                                         const double* __restrict__ decode, const uint8_t* __restrict__ encode, int T,
                                                         int H, int W, uint32_t* __restrict__ rgba, float* __restrict__ zdepth,
                                                         int* __restrict__ unlit)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (p >= (unsigned)H * (unsigned)W) return;
    const size_t o = (size_t)n * H * W + p;
    uint32_t px = 0u;
    Pixel pixel;
    resolve_pixel(vis[o], p, xy + 2 * (size_t)n * V, depth + (size_t)n * V, V, faces, F, H, W, pixel, [&](const Pixel& pix) {
        const Tri& t = pix.t;
        const double t0 = pix.t0, t1 = pix.t1, t2 = pix.t2;
        double g[3];
        if (kFlat) {
            const int i1 = t.swapped ? t.i2 : t.i1, i2 = t.swapped ? t.i1 : t.i2;   // the stored order
            face_cross(vertices, t.i0, i1, i2, g);
        } else {
            const double *n0 = normals + 3 * (size_t)t.i0, *n1 = normals + 3 * (size_t)t.i1, *n2 = normals + 3 * (size_t)t.i2;
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = (t0 * n0[k] + t1 * n1[k]) + t2 * n2[k];
        }
        const float* P = poses + 16 * (size_t)n;
        double m[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) m[r] = ((double)P[4 * r] * g[0] + (double)P[4 * r + 1] * g[1]) + (double)P[4 * r + 2] * g[2];
        const double z = (double)pix.z;
        const double yn = ((double)pix.y - S.K5) / S.K4;
        const double xn = (((double)pix.x - S.K2) - S.K1 * yn) / S.K0;
        const double pos[3] = {xn * z, yn * z, z};
        const double s = (m[0] * pos[0] + m[1] * pos[1]) + m[2] * pos[2];
        if (s > 0.0) m[0] = -m[0], m[1] = -m[1], m[2] = -m[2];
        const double mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
        double E = S.ambient;
        if (mm > 0.0 && mm < kInf) {
            for (int l = 0; l < S.L; ++l) {
                const double d0 = S.light[l][0] - pos[0], d1 = S.light[l][1] - pos[1], d2 = S.light[l][2] - pos[2];
                const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                const double md = (m[0] * d0 + m[1] * d1) + m[2] * d2;
                if (md > 0.0 && dd > 0.0) E = E + (S.light[l][3] * md) / (root(mm * dd) * dd);
            }
        } else {
            atomicAdd(unlit + n, 1);
        }
        const double top = (double)(T - 1);
        px = 0xff000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double w = floor((decode[vertex_colour_byte(colours, pix, c)] * E) * top + 0.5);
            const unsigned i = w >= top ? (unsigned)(T - 1) : (w > 0.0 ? (unsigned)w : 0u);   // a NaN fails both: 0
            px |= (uint32_t)encode[i] << (8 * c);
        }
    });
    rgba[o] = px;
    zdepth[o] = pixel.z;
}

bool finite_host(double x) { return x == x && x - x == 0.0; }

}  // namespace

extern "C" {

int gpl_abi_version(void) { return 1; }

int gpl_vertex_normals(const float* vertices, int V, const int* faces, int F, double unit, long long* acc, int* flags, double* normals,
                       void* stream)
{
    GPF_REQUIRE(V >= 1 && F >= 0, "gpl_vertex_normals: bad sizes (V >= 1, F >= 0)");
    GPF_REQUIRE(finite_host(unit) && unit > 0.0, "gpl_vertex_normals: unit must be finite and > 0 (a power of two)");
    GPF_REQUIRE(vertices && acc && flags && normals && (faces || F == 0), "gpl_vertex_normals: null pointer");
    GPF_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)normals & 7) == 0, "gpl_vertex_normals: acc or normals is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpl_vertex_normals", hipMemsetAsync(acc, 0, (size_t)V * 3 * sizeof(long long), s));
    GPF_CHECK_HIP("gpl_vertex_normals", hipMemsetAsync(flags, 0, (size_t)V * sizeof(int), s));
    if (F > 0) {
        hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)(((long long)F + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, vertices, V,
                           faces, F, unit, reinterpret_cast<unsigned long long*>(acc), flags);
        GPF_CHECK_LAUNCH("gpl_vertex_normals");
    }
    hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)(((long long)V + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, acc, V, flags,
                       normals);
    GPF_CHECK_LAUNCH("gpl_vertex_normals");
    return GPF_OK;
}

int gpl_shade(const unsigned long long* vis, const int* xy, const float* depth, int V, const int* faces, int F, const uint8_t* colours,
              const float* vertices, const double* normals, const float* poses, const float* K_host, const double* lights_host, int L,
              double ambient, const double* decode, const uint8_t* encode, int T, int mode, int N, int H, int W, uint8_t* rgba,
              float* zdepth, int* unlit, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W) && V >= 0 && F >= 0, "gpl_shade: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31, V, F >= 0)");
    GPF_REQUIRE(L >= 0 && L <= GPL_MAX_LIGHTS, "gpl_shade: bad number of lights (0 <= L <= 16)");
    GPF_REQUIRE(T >= 256 && T <= 65536, "gpl_shade: bad table size (256 <= T <= 65536)");
    GPF_REQUIRE(mode == GPL_SMOOTH || mode == GPL_FLAT, "gpl_shade: mode must be GPL_SMOOTH or GPL_FLAT");
    GPF_REQUIRE(K_host && (lights_host || L == 0), "gpl_shade: null host pointer");
    GPF_REQUIRE(K_host[0] != 0.0f && K_host[4] != 0.0f, "gpl_shade: K[0] and K[4] must not be 0");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && rgba && zdepth && unlit && poses && decode && encode, "gpl_shade: null pointer");
    GPF_REQUIRE(F == 0 || (xy && depth && faces && colours && (mode == GPL_FLAT ? (const void*)vertices : (const void*)normals)),
                "gpl_shade: null pointer");
    GPF_REQUIRE(((uintptr_t)rgba & 3) == 0, "gpl_shade: rgba is not 4-byte aligned (one pixel is one word)");
    GPF_REQUIRE(((uintptr_t)decode & 7) == 0 && ((uintptr_t)normals & 7) == 0, "gpl_shade: normals or decode is not 8-byte aligned");
    Scene S;
    S.K0 = (double)K_host[0], S.K1 = (double)K_host[1], S.K2 = (double)K_host[2], S.K4 = (double)K_host[4], S.K5 = (double)K_host[5];
    S.ambient = ambient;
    S.L = L;
    for (int l = 0; l < GPL_MAX_LIGHTS; ++l)
        for (int k = 0; k < 4; ++k) S.light[l][k] = l < L ? lights_host[4 * l + k] : 0.0;
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpl_shade", hipMemsetAsync(unlit, 0, (size_t)N * sizeof(int), s));
    const unsigned blocks = (unsigned)(((long long)H * W + kThreads - 1) / kThreads);
    uint32_t* out = reinterpret_cast<uint32_t*>(rgba);
    if (mode == GPL_FLAT)
        hipLaunchKernelGGL(shade_kernel<true>, dim3(blocks, N), dim3(kThreads), 0, s, vis, xy, depth, V, faces, F, colours, vertices, normals,
                           poses, S, decode, encode, T, H, W, out, zdepth, unlit);
    else
        hipLaunchKernelGGL(shade_kernel<false>, dim3(blocks, N), dim3(kThreads), 0, s, vis, xy, depth, V, faces, F, colours, vertices, normals,
                           poses, S, decode, encode, T, H, W, out, zdepth, unlit);
    GPF_CHECK_LAUNCH("gpl_shade");
    return GPF_OK;
}

}  // extern "C"
