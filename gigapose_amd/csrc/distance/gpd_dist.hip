// libgigapose_dist.so (C-ABI: include/gigapose_dist.h): all-pairs vertex distances -- ADD and ADD-S of N (estimate, ground
// truth) pairs as integer sums of quantised distances, and the square of the model diameter.
//   reference: src/lib3d/metric.py is ADD in torch; nothing of it is restated here, the header's definitions are the contract.
// add_kernel<kSym>, grid (chunk of 1024 query vertices, pair): a thread keeps 4 ground-truth points g_i and their running minima
// in registers.  kSym: the estimate points e_j are transformed once per workgroup while they are staged through LDS in tiles of
// 1024 (structure of arrays, doubles, 24 KB); every lane reads the same address in the inner loop, so the reads broadcast:
// 9 float64 vector operations per point pair, 3 LDS reads per staged point and thread.  The inner loop is bounded by the number
// of points staged, never by padding values.  !kSym: the same skeleton without the inner loop.  Then root, scale, rint and an
// integer sum: wave shuffles, LDS, one 64-bit atomic add and at most one atomic OR per workgroup.
// diameter_kernel, grid (chunk i, chunk j), the tiles below the diagonal return at once: the same inner loop with a maximum;
// a tile on the diagonal takes j > i only.  One 64-bit unsigned atomic maximum per workgroup.
// Only integers are merged, so no result depends on the order of arrival.  gigapose_testing/dist_ref.py restates the arithmetic
// in numpy; the two agree bit for bit.
// The host-side plumbing is gp_front.h's.  This library links no object of the other libraries and exports only gpd_* names.
#include <float.h>
#include <math.h>

#include "gigapose_dist.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpd
#include "../gp_front.h"
#include "../gp_root.h"    // root(): the correctly rounded square root, the library's one fused operation (the header)

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQ = 4;                    // query points a thread keeps in registers
constexpr int kChunk = kThreads * kQ;    // query points of a workgroup
constexpr int kTile = 1024;              // points staged in LDS at a time: 3 x 8 KB
constexpr int kMaxV = 1 << 20;
constexpr u64 kBadKey = ~0ull;
static_assert(kTile == kChunk, "the diameter kernel pairs query chunks with staged tiles");

__device__ __forceinline__ bool finite(double x) { return fabs(x) <= DBL_MAX; }

struct Rows {
    double m[12];
    __device__ __forceinline__ void load(const double* p)
    {
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = p[i];
    }
    __device__ __forceinline__ void apply(double x, double y, double z, double& ox, double& oy, double& oz) const
    {
        ox = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        oy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        oz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    }
};

__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz)
{
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// grid (ceil(V / 1024), N).  sums (N), status (N): zeroed by the caller
template <bool kSym>
__global__ __launch_bounds__(kThreads) void add_kernel(const float* __restrict__ vertices, int V, const double* __restrict__ est,
                                                       const double* __restrict__ gt, double scale, long long* __restrict__ sums,
                                                       int* __restrict__ status)
{
    __shared__ double sx[kSym ? kTile : 1], sy[kSym ? kTile : 1], sz[kSym ? kTile : 1];
    __shared__ long long part[kWaves];
    __shared__ int bad_part[kWaves];
    const int n = blockIdx.y, tid = threadIdx.x;
    Rows P, G;
    P.load(est + 16 * (size_t)n);
    G.load(gt + 16 * (size_t)n);
    double gx[kQ], gy[kQ], gz[kQ], m[kQ];
    bool live[kQ];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        int v = (blockIdx.x * kQ + k) * kThreads + tid;                 // < 2^20 + 1024
        live[k] = v < V;
        if (!live[k]) v = V - 1;         // a lane past the end repeats the last vertex and adds nothing
        const double x = vertices[3 * (size_t)v + 0], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
        G.apply(x, y, z, gx[k], gy[k], gz[k]);
        if (!(finite(gx[k]) && finite(gy[k]) && finite(gz[k]))) bad |= 1;
        if (kSym) {
            m[k] = (double)INFINITY;
        } else {
            double ex, ey, ez;
            P.apply(x, y, z, ex, ey, ez);
            if (!(finite(ex) && finite(ey) && finite(ez))) bad |= 1;
            m[k] = dist2(ex, ey, ez, gx[k], gy[k], gz[k]);
        }
    }
    if (kSym) {
        for (int t0 = 0; t0 < V; t0 += kTile) {
            __syncthreads();             // the readers of the previous tile are done
#pragma unroll
            for (int k = 0; k < kTile / kThreads; ++k) {
                const int slot = k * kThreads + tid, j = t0 + slot;
                if (j < V) {
                    const double x = vertices[3 * (size_t)j + 0], y = vertices[3 * (size_t)j + 1], z = vertices[3 * (size_t)j + 2];
                    double ex, ey, ez;
                    P.apply(x, y, z, ex, ey, ez);
                    if (!(finite(ex) && finite(ey) && finite(ez))) bad |= 1;
                    sx[slot] = ex, sy[slot] = ey, sz[slot] = ez;
                }
            }
            __syncthreads();
            const int cnt = min(kTile, V - t0);                         // the slots that were written: nothing past them is read
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
                const double ex = sx[j], ey = sy[j], ez = sz[j];        // one address for the whole wave: a broadcast
#pragma unroll
                for (int k = 0; k < kQ; ++k) m[k] = fmin(m[k], dist2(gx[k], gy[k], gz[k], ex, ey, ez));
            }
        }
    }
    long long sum = 0;
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        if (!live[k]) continue;
        if (!(m[k] < (double)INFINITY)) bad |= 1;
        const double s = root(m[k]) * scale;
        if (s < 0x1p42) sum += (long long)rint(s);
        else bad |= 2;
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        sum += __shfl_xor(sum, w, 64);
        bad |= __shfl_xor(bad, w, 64);
    }
    if ((tid & 63) == 0) part[tid >> 6] = sum, bad_part[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) sum += part[w], bad |= bad_part[w];
        if (sum) atomicAdd(reinterpret_cast<u64*>(sums) + n, (u64)sum);   // one atomic per workgroup; the result is not used
        if (bad) atomicOr(status + n, bad);
    }
}

// one staged tile against a thread's query points.  kUpper: a tile on the diagonal, where only j > i counts
template <bool kUpper>
__device__ __forceinline__ void sweep_max(const double* sx, const double* sy, const double* sz, int cnt, int j0, const double (&qx)[kQ],
                                          const double (&qy)[kQ], const double (&qz)[kQ], const int (&qi)[kQ], double (&m)[kQ])
{
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
        const double x = sx[j], y = sy[j], z = sz[j];
#pragma unroll
        for (int k = 0; k < kQ; ++k) {
            const double d2 = dist2(qx[k], qy[k], qz[k], x, y, z);
            m[k] = (!kUpper || j0 + j > qi[k]) ? fmax(m[k], d2) : m[k];
        }
    }
}

// grid (C, C), C = ceil(V / 1024): workgroup (bi, bj), bi <= bj, takes query chunk bi against staged chunk bj.  key zeroed by the caller
__global__ __launch_bounds__(kThreads) void diameter_kernel(const float* __restrict__ vertices, int V, u64* __restrict__ key)
{
    __shared__ double sx[kTile], sy[kTile], sz[kTile];
    __shared__ u64 part[kWaves];
    const int bi = blockIdx.x, bj = blockIdx.y, tid = threadIdx.x;
    if (bj < bi) return;                 // uniform over the workgroup
    double qx[kQ], qy[kQ], qz[kQ], m[kQ];
    int qi[kQ];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        int v = (bi * kQ + k) * kThreads + tid;
        if (v >= V) v = V - 1;           // a lane past the end repeats the last vertex: a maximum does not change
        qi[k] = v;
        qx[k] = vertices[3 * (size_t)v + 0], qy[k] = vertices[3 * (size_t)v + 1], qz[k] = vertices[3 * (size_t)v + 2];
        if (!(finite(qx[k]) && finite(qy[k]) && finite(qz[k]))) bad = true;
        m[k] = 0.0;
    }
    const int j0 = bj * kTile;
#pragma unroll
    for (int k = 0; k < kTile / kThreads; ++k) {
        const int slot = k * kThreads + tid, j = j0 + slot;
        if (j < V) {
            const double x = vertices[3 * (size_t)j + 0], y = vertices[3 * (size_t)j + 1], z = vertices[3 * (size_t)j + 2];
            if (!(finite(x) && finite(y) && finite(z))) bad = true;
            sx[slot] = x, sy[slot] = y, sz[slot] = z;
        }
    }
    __syncthreads();
    const int cnt = min(kTile, V - j0);  // >= 1: bj < C
    if (bi == bj) sweep_max<true>(sx, sy, sz, cnt, j0, qx, qy, qz, qi, m);
    else sweep_max<false>(sx, sy, sz, cnt, j0, qx, qy, qz, qi, m);
    // finite f32 coordinates: no d2 overflows and none is a NaN, so the maximum of doubles is exact; a coordinate that is not
    // finite makes every d2 it enters +inf or a NaN, which is the key of all ones as soon as there is a pair at all
    double best = fmax(fmax(m[0], m[1]), fmax(m[2], m[3]));
    u64 kmax = (bad && V >= 2) ? kBadKey : (u64)__double_as_longlong(best);
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const u64 o = __shfl_xor(kmax, w, 64);
        kmax = o > kmax ? o : kmax;
    }
    if ((tid & 63) == 0) part[tid >> 6] = kmax;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) kmax = part[w] > kmax ? part[w] : kmax;
        atomicMax(key, kmax);            // one atomic per workgroup; the result is not used
    }
}

__global__ __launch_bounds__(kThreads) void root_kernel(const double* __restrict__ x, long long n, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = root(x[i]);
}

template <bool kSym>
int launch_add(const char* name, const float* vertices, int V, const double* est, const double* gt, int N, int k, long long* sums,
               int* status, void* stream)
{
    if (!(V >= 1 && V <= kMaxV && N >= 0 && N <= 65535)) {
        set_error("%s: bad sizes (1 <= V <= 2^20, 0 <= N <= 65535)", name);
        return GPF_EINVAL;
    }
    if (!(k >= -64 && k <= 64)) {
        set_error("%s: k must be in [-64, 64]", name);
        return GPF_EINVAL;
    }
    if (N == 0) return GPF_OK;
    if (!(vertices && est && gt && sums && status)) {
        set_error("%s: null pointer", name);
        return GPF_EINVAL;
    }
    if (((uintptr_t)sums & 7) != 0) {
        set_error("%s: sums is not 8-byte aligned", name);
        return GPF_EINVAL;
    }
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP(name, hipMemsetAsync(sums, 0, (size_t)N * sizeof(long long), s));
    GPF_CHECK_HIP(name, hipMemsetAsync(status, 0, (size_t)N * sizeof(int), s));
    hipLaunchKernelGGL(add_kernel<kSym>, dim3((V + kChunk - 1) / kChunk, N), dim3(kThreads), 0, s, vertices, V, est, gt, ldexp(1.0, k),
                       sums, status);
    GPF_CHECK_LAUNCH(name);
    return GPF_OK;
}

}  // namespace

extern "C" {

int gpd_abi_version(void) { return 1; }

int gpd_add(const float* vertices, int V, const double* est, const double* gt, int N, int k, long long* sums, int* status, void* stream)
{
    return launch_add<false>("gpd_add", vertices, V, est, gt, N, k, sums, status, stream);
}

int gpd_adds(const float* vertices, int V, const double* est, const double* gt, int N, int k, long long* sums, int* status, void* stream)
{
    return launch_add<true>("gpd_adds", vertices, V, est, gt, N, k, sums, status, stream);
}

int gpd_diameter2(const float* vertices, int V, unsigned long long* key, void* stream)
{
    GPF_REQUIRE(V >= 1 && V <= kMaxV, "gpd_diameter2: bad sizes (1 <= V <= 2^20)");
    GPF_REQUIRE(vertices && key, "gpd_diameter2: null pointer");
    GPF_REQUIRE(((uintptr_t)key & 7) == 0, "gpd_diameter2: key is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpd_diameter2", hipMemsetAsync(key, 0, sizeof(u64), s));
    const unsigned C = (unsigned)((V + kTile - 1) / kTile);
    hipLaunchKernelGGL(diameter_kernel, dim3(C, C), dim3(kThreads), 0, s, vertices, V, key);
    GPF_CHECK_LAUNCH("gpd_diameter2");
    return GPF_OK;
}

int gpd_root(const double* x, long long n, double* out, void* stream)
{
    GPF_REQUIRE(n >= 0 && n < (1ll << 31), "gpd_root: bad size (0 <= n < 2^31)");
    if (n == 0) return GPF_OK;
    GPF_REQUIRE(x && out, "gpd_root: null pointer");
    hipLaunchKernelGGL(root_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, x, n, out);
    GPF_CHECK_LAUNCH("gpd_root");
    return GPF_OK;
}

}  // extern "C"
