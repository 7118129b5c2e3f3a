// libgigapose_eval.so (C-ABI: include/gigapose_eval.h): the BOP-19 pose errors of N (estimate, ground truth) pairs -- MSSD and
// MSPD over every symmetry transform and every vertex, and VSD as integer counts over three depth maps per pair.
//   reference: src/scripts/eval_bop.py:29 shells out to bop_toolkit (vispy / OpenGL); nothing of it is restated here, the
//   header's definitions are the contract.
// gpe_mssd_mspd: sym_poses_kernel writes G = gt * sym per (pair, symmetry); deviation_kernel, grid (vertex chunk, pair), keeps
// its vertices transformed by the estimate in registers, walks the symmetries, reduces each one's two maxima by wave shuffles,
// through LDS, and merges one value per workgroup into an (N,S,2) buffer of keys with a 64-bit unsigned atomic maximum (a
// non-negative double orders like its bits; anything not below +inf takes the key of all ones, so a NaN wins); finish_kernel
// takes the minimum over the symmetries.  gpe_vsd_counts: a thread counts over 8 pixels, a workgroup adds its 2 + T counters
// once.  Only integers are merged, so no result depends on the order of arrival.  gigapose_testing/eval_ref.py restates the
// arithmetic in numpy; the two agree bit for bit.
// The host-side plumbing is gp_front.h's.  This library links no object of the other libraries and exports only gpe_* names.
#include <float.h>
#include <math.h>

#include "gigapose_eval.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpe
#include "../gp_front.h"

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kVerts = 4;                // vertices a thread keeps in registers: a workgroup covers 1024
constexpr int kPixels = 8;               // pixels a thread counts over: a workgroup covers 2048
constexpr int kMaxThr = 16;              // GPE_MAX_THRESHOLDS
constexpr u64 kBadKey = ~0ull;

__device__ __forceinline__ u64 key_of(double x) { return x < (double)INFINITY ? (u64)__double_as_longlong(x) : kBadKey; }   // x >= 0 or NaN
__device__ __forceinline__ u64 max_u64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 min_u64(u64 a, u64 b) { return a < b ? a : b; }

__device__ __forceinline__ u64 wave_max(u64 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max_u64(v, __shfl_xor(v, m, 64));
    return v;
}

// grid (ceil(S / 256), N): thread = (pair, symmetry) -> the 12 doubles of rows 0..2 of gt[n] * syms[s]
__global__ __launch_bounds__(kThreads) void sym_poses_kernel(const double* __restrict__ gt, const double* __restrict__ syms, int S,
                                                             double* __restrict__ G)
{
    const int s = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.y;
    if (s >= S) return;
    const double* g = gt + 16 * (size_t)n;
    const double* m = syms + 16 * (size_t)s;
    double* out = G + 12 * ((size_t)n * S + s);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double g0 = g[4 * i + 0], g1 = g[4 * i + 1], g2 = g[4 * i + 2], g3 = g[4 * i + 3];
#pragma unroll
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (g0 * m[j] + g1 * m[4 + j]) + g2 * m[8 + j];
        out[4 * i + 3] = ((g0 * m[3] + g1 * m[7]) + g2 * m[11]) + g3;
    }
}

// grid (ceil(V / 1024), N).  keys (N,S,2): [0] the maximum of d2, [1] of p2, zeroed by the caller
__global__ __launch_bounds__(kThreads) void deviation_kernel(const float* __restrict__ vertices, int V, const double* __restrict__ est,
                                                             const double* __restrict__ K, const double* __restrict__ G, int S,
                                                             double zmin, u64* __restrict__ keys)
{
    __shared__ u64 part[2][kWaves][2];
    const int n = blockIdx.y, tid = threadIdx.x;
    const double* P = est + 16 * (size_t)n;
    const double* Kn = K + 9 * (size_t)n;
    const double k0 = Kn[0], k1 = Kn[1], k2 = Kn[2], k3 = Kn[3], k4 = Kn[4], k5 = Kn[5];
    double x[kVerts], y[kVerts], z[kVerts], ex[kVerts], ey[kVerts], ez[kVerts], eu[kVerts], ev[kVerts];
#pragma unroll
    for (int k = 0; k < kVerts; ++k) {
        long long v = ((long long)blockIdx.x * kVerts + k) * kThreads + tid;
        if (v >= V) v = V - 1;           // a lane past the end repeats the last vertex: a maximum does not change
        x[k] = vertices[3 * (size_t)v + 0], y[k] = vertices[3 * (size_t)v + 1], z[k] = vertices[3 * (size_t)v + 2];
        ex[k] = ((P[0] * x[k] + P[1] * y[k]) + P[2] * z[k]) + P[3];
        ey[k] = ((P[4] * x[k] + P[5] * y[k]) + P[6] * z[k]) + P[7];
        ez[k] = ((P[8] * x[k] + P[9] * y[k]) + P[10] * z[k]) + P[11];
        eu[k] = ((k0 * ex[k] + k1 * ey[k]) + k2 * ez[k]) / ez[k];
        ev[k] = ((k3 * ex[k] + k4 * ey[k]) + k5 * ez[k]) / ez[k];
    }
    for (int s = 0; s < S; ++s) {
        const double* g = G + 12 * ((size_t)n * S + s);   // uniform over the workgroup
        u64 kd = 0, kp = 0;
#pragma unroll
        for (int k = 0; k < kVerts; ++k) {
            const double gx = ((g[0] * x[k] + g[1] * y[k]) + g[2] * z[k]) + g[3];
            const double gy = ((g[4] * x[k] + g[5] * y[k]) + g[6] * z[k]) + g[7];
            const double gz = ((g[8] * x[k] + g[9] * y[k]) + g[10] * z[k]) + g[11];
            const double dx = ex[k] - gx, dy = ey[k] - gy, dz = ez[k] - gz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const double gu = ((k0 * gx + k1 * gy) + k2 * gz) / gz;
            const double gv = ((k3 * gx + k4 * gy) + k5 * gz) / gz;
            const double du = eu[k] - gu, dv = ev[k] - gv;
            const double p2 = du * du + dv * dv;
            kd = max_u64(kd, key_of(d2));
            kp = max_u64(kp, (ez[k] < zmin || gz < zmin) ? kBadKey : key_of(p2));
        }
        kd = wave_max(kd);
        kp = wave_max(kp);
        const int b = s & 1;             // two buffers: one barrier per symmetry
        if ((tid & 63) == 0) part[b][tid >> 6][0] = kd, part[b][tid >> 6][1] = kp;
        __syncthreads();
        if (tid < 2) {
            u64 m = part[b][0][tid];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) m = max_u64(m, part[b][w][tid]);
            atomicMax(keys + 2 * ((size_t)n * S + s) + tid, m);   // one atomic per workgroup and value; the result is not used
        }
    }
}

// grid (N), one wave: the minimum over the symmetries; a key of all ones anywhere gives +inf
__global__ __launch_bounds__(64) void finish_kernel(const u64* __restrict__ keys, int S, double* __restrict__ mssd2, double* __restrict__ mspd2)
{
    const int n = blockIdx.x;
    u64 lo[2] = {kBadKey, kBadKey}, hi[2] = {0, 0};
    for (int s = threadIdx.x; s < S; s += 64) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const u64 k = keys[2 * ((size_t)n * S + s) + c];
            lo[c] = min_u64(lo[c], k);
            hi[c] = max_u64(hi[c], k);
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) lo[c] = min_u64(lo[c], __shfl_xor(lo[c], m, 64));
        hi[c] = wave_max(hi[c]);
    }
    if (threadIdx.x == 0) {
        mssd2[n] = hi[0] == kBadKey ? (double)INFINITY : __longlong_as_double((long long)lo[0]);
        mspd2[n] = hi[1] == kBadKey ? (double)INFINITY : __longlong_as_double((long long)lo[1]);
    }
}

__device__ __forceinline__ float clean_depth(float d) { return (d > 0.0f && d <= FLT_MAX) ? d : 0.0f; }   // negative, NaN, inf -> nothing

// grid (ceil(H*W / 2048), N).  counts (N, 2+T), zeroed by the caller
__global__ __launch_bounds__(kThreads) void vsd_kernel(const float* __restrict__ depth_est, const float* __restrict__ depth_gt,
                                                       const float* __restrict__ depth_test, int M, const int* __restrict__ frame,
                                                       const double* __restrict__ ray, int R, const int* __restrict__ ray_index,
                                                       unsigned HW, double delta, const double* __restrict__ thr, int T,
                                                       long long* __restrict__ counts)
{
    __shared__ unsigned part[kWaves][2 + kMaxThr];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int fi = frame[n], ri = ray_index[n];
    if (fi < 0 || fi >= M || ri < 0 || ri >= R) {   // uniform over the workgroup
        if (blockIdx.x == 0 && tid == 0) counts[(size_t)n * (2 + T)] = -1;
        return;
    }
    const float* de_n = depth_est + (size_t)n * HW;
    const float* dg_n = depth_gt + (size_t)n * HW;
    const float* dt_n = depth_test + (size_t)fi * HW;
    const double* ray_n = ray + (size_t)ri * HW;
    double th[kMaxThr];
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) th[t] = t < T ? thr[(size_t)n * T + t] : 0.0;
    unsigned c[2 + kMaxThr];
#pragma unroll
    for (int t = 0; t < 2 + kMaxThr; ++t) c[t] = 0u;
#pragma unroll
    for (int k = 0; k < kPixels; ++k) {
        const size_t p = ((size_t)blockIdx.x * kPixels + k) * kThreads + tid;
        if (p >= HW) continue;
        const float de = clean_depth(de_n[p]), dg = clean_depth(dg_n[p]), dt = clean_depth(dt_n[p]);
        const double r = ray_n[p];
        const double De = (double)de * r, Dg = (double)dg * r, Dt = (double)dt * r;
        const bool vis_gt = (dg > 0.0f && dt > 0.0f && (Dg - Dt) <= delta) || (dg > 0.0f && dt == 0.0f);
        const bool vis_est = (de > 0.0f && dt > 0.0f && (De - Dt) <= delta) || (de > 0.0f && dt == 0.0f) || (vis_gt && de > 0.0f);
        const bool inter = vis_gt && vis_est;
        c[0] += (vis_gt || vis_est) ? 1u : 0u;
        c[1] += inter ? 1u : 0u;
        const double cost = fabs(Dg - De);
#pragma unroll
        for (int t = 0; t < kMaxThr; ++t) c[2 + t] += (inter && t < T && cost >= th[t]) ? 1u : 0u;
    }
#pragma unroll
    for (int t = 0; t < 2 + kMaxThr; ++t) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c[t] += __shfl_xor(c[t], m, 64);
        if ((tid & 63) == 0) part[tid >> 6][t] = c[t];
    }
    __syncthreads();
    if (tid < 2 + T) {
        unsigned sum = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += part[w][tid];            // <= 2048
        if (sum) atomicAdd(reinterpret_cast<u64*>(counts) + (size_t)n * (2 + T) + tid, (u64)sum);   // one atomic per workgroup and counter
    }
}

}  // namespace

extern "C" {

int gpe_abi_version(void) { return 1; }

size_t gpe_pose_workspace_bytes(int N, int S)
{
    if (N < 0 || S < 0) return 0;
    return (size_t)N * (size_t)S * (12 + 2) * sizeof(double);
}

int gpe_mssd_mspd(const float* vertices, int V, const double* syms, int S, const double* est, const double* gt, const double* K,
                  int N, double zmin, double* mssd2, double* mspd2, void* workspace, void* stream)
{
    GPF_REQUIRE(V >= 1 && S >= 1 && N >= 0 && N <= 65535, "gpe_mssd_mspd: bad sizes (V >= 1, S >= 1, 0 <= N <= 65535)");
    GPF_REQUIRE(zmin >= -DBL_MAX && zmin <= DBL_MAX, "gpe_mssd_mspd: zmin must be finite");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vertices && syms && est && gt && K && mssd2 && mspd2 && workspace, "gpe_mssd_mspd: null pointer");
    GPF_REQUIRE(((uintptr_t)workspace & 7) == 0, "gpe_mssd_mspd: workspace is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const size_t pairs = (size_t)N * (size_t)S;
    u64* keys = reinterpret_cast<u64*>(workspace);
    double* G = reinterpret_cast<double*>(workspace) + 2 * pairs;
    GPF_CHECK_HIP("gpe_mssd_mspd", hipMemsetAsync(keys, 0, 2 * pairs * sizeof(u64), s));
    hipLaunchKernelGGL(sym_poses_kernel, dim3((S + kThreads - 1) / kThreads, N), dim3(kThreads), 0, s, gt, syms, S, G);
    GPF_CHECK_LAUNCH("gpe_mssd_mspd");
    const int chunk = kThreads * kVerts;
    hipLaunchKernelGGL(deviation_kernel, dim3((unsigned)(((long long)V + chunk - 1) / chunk), N), dim3(kThreads), 0, s, vertices, V, est,
                       K, G, S, zmin, keys);
    GPF_CHECK_LAUNCH("gpe_mssd_mspd");
    hipLaunchKernelGGL(finish_kernel, dim3(N), dim3(64), 0, s, keys, S, mssd2, mspd2);
    GPF_CHECK_LAUNCH("gpe_mssd_mspd");
    return GPF_OK;
}

int gpe_vsd_counts(const float* depth_est, const float* depth_gt, int N, const float* depth_test, int M, const int* frame,
                   const double* ray, int R, const int* ray_index, int H, int W, double delta, const double* thr, int T,
                   long long* counts, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(N, H, W) && M >= 1 && R >= 1, "gpe_vsd_counts: bad sizes (0 <= N <= 65535, H, W > 0, H*W < 2^31, M, R >= 1)");
    GPF_REQUIRE(T >= 1 && T <= kMaxThr, "gpe_vsd_counts: T must be in [1, 16]");
    GPF_REQUIRE(delta == delta, "gpe_vsd_counts: delta is NaN");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(depth_est && depth_gt && depth_test && frame && ray && ray_index && thr && counts, "gpe_vsd_counts: null pointer");
    GPF_REQUIRE(((uintptr_t)counts & 7) == 0, "gpe_vsd_counts: counts is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const unsigned HW = (unsigned)H * (unsigned)W;
    GPF_CHECK_HIP("gpe_vsd_counts", hipMemsetAsync(counts, 0, (size_t)N * (2 + T) * sizeof(long long), s));
    const unsigned per = kThreads * kPixels;
    hipLaunchKernelGGL(vsd_kernel, dim3((HW + per - 1) / per, N), dim3(kThreads), 0, s, depth_est, depth_gt, depth_test, M, frame, ray, R,
                       ray_index, HW, delta, thr, T, counts);
    GPF_CHECK_LAUNCH("gpe_vsd_counts");
    return GPF_OK;
}

}  // extern "C"
