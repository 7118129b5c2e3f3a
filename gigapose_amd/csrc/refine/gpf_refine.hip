// libgigapose_refine.so (C-ABI: include/gigapose_refine.h): point-to-plane ICP of pose estimates against the sensor's depth,
// with same-pixel association on the render library's z-buffer of 64-bit keys.
//   reference: the role of src/megapose/inference/icp_refiner.py (render, compare with the measured depth, move the pose, keep
//   the input on failure); nothing of it is restated here, the header's definitions are the contract.
// accumulate_kernel walks the pair's box as gp_key_walk.h states it: grid (chunk of 4096 box pixels, pair); a workgroup whose chunk
// lies beyond the pair's clamped box returns before it reads a key, or the pair's frame.  A thread keeps the 30 integer sums of its
// 16 pixels in registers (every term is quantised before it is added), then the header's wave and workgroup sums, and ONE 32-lane
// atomic add of int64 into the pair's 256-byte row per workgroup that saw a covered pixel, at most one atomic OR for the status.
// No float atomics.
// update_kernel: one thread per pair -- 6 x 6 LDL^T, the Cayley transform, the new pose as f64 and f32.
// No square root and no transcendental function.  gigapose_testing/refine_ref.py restates the arithmetic in numpy; the two agree
// bit for bit.  The host-side plumbing is gp_front.h's.  This library links no object of the other libraries and exports only
// gpf_* names.
#include <float.h>
#include <math.h>

#include "gigapose_refine.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpf
#include "../gp_front.h"
#include "../gp_key_walk.h"

namespace {

constexpr int kTerms = 28;                    // 21 + 6 + 1
constexpr int kLive = 30;                     // + covered, count
static_assert(GPF_SUMS == 32 && GPF_SUM_COUNT == kLive - 1 && GPF_SUM_EE == kTerms - 1, "the layout of a row of sums");

// (int64) rint(v) for |v| < 2^51: v + 1.5 * 2^52 is v rounded half to even to an integer, held in the low bits of the sum
__device__ __forceinline__ long long quantise(double term)
{
    const double magic = 0x1.8p52;
    return __double_as_longlong(term * 0x1p36 + magic) - __double_as_longlong(magic);
}

__global__ __launch_bounds__(kThreads) void face_normals_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces,
                                                                int F, double* __restrict__ c)
{
    const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * (size_t)f + 0], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    double c0 = (double)NAN, c1 = (double)NAN, c2 = (double)NAN;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float *p0 = vertices + 3 * (size_t)i0, *p1 = vertices + 3 * (size_t)i1, *p2 = vertices + 3 * (size_t)i2;
        const double u0 = (double)p1[0] - (double)p0[0], u1 = (double)p1[1] - (double)p0[1], u2 = (double)p1[2] - (double)p0[2];
        const double v0 = (double)p2[0] - (double)p0[0], v1 = (double)p2[1] - (double)p0[1], v2 = (double)p2[2] - (double)p0[2];
        c0 = u1 * v2 - u2 * v1, c1 = u2 * v0 - u0 * v2, c2 = u0 * v1 - u1 * v0;
    }
    c[3 * (size_t)f + 0] = c0, c[3 * (size_t)f + 1] = c1, c[3 * (size_t)f + 2] = c2;
}

// grid (ceil(H*W / 4096), N).  sums (N,32), status (N): zeroed by the caller
__global__ __launch_bounds__(kThreads) void accumulate_kernel(const u64* __restrict__ vis, const double* __restrict__ c, int F,
                                                              const double* __restrict__ poses, const double* __restrict__ K,
                                                              const float* __restrict__ depth, int M, const int* __restrict__ frame,
                                                              const int* __restrict__ box, const double* __restrict__ gate,
                                                              const double* __restrict__ scale, int H, int W, long long* __restrict__ sums,
                                                              int* __restrict__ status)
{
    __shared__ long long part[kWaves][kLive];
    __shared__ int bad_part[kWaves];
    const int n = blockIdx.y, tid = threadIdx.x;
    BoxWalk walk;
    if (!walk.open(box, n, H, W)) return;                   // uniform over the workgroup, like every return below; no status is set
    const int fr = frame[n];
    if (fr < 0 || fr >= M) {
        if (tid == 0 && blockIdx.x == 0) atomicOr(status + n, GPF_BAD_INDEX);
        return;
    }
    const double* P = poses + 16 * (size_t)n;
    const double R00 = P[0], R01 = P[1], R02 = P[2], t0 = P[3], R10 = P[4], R11 = P[5], R12 = P[6], t1 = P[7], R20 = P[8], R21 = P[9],
                 R22 = P[10], t2 = P[11];
    const double* k = K + 9 * (size_t)n;
    const double k0 = k[0], k1 = k[1], k2 = k[2], k4 = k[4], k5 = k[5];
    const double gt = gate[n], sc = scale[n];
    const u64* keys = vis + (size_t)n * H * W;
    const float* dmap = depth + (size_t)fr * H * W;

    long long acc[kLive];
#pragma unroll
    for (int i = 0; i < kLive; ++i) acc[i] = 0;
    int bad = 0;
    walk.for_each(W, [&](int px, int py, size_t at) {
        const u64 key = keys[at];
        if (key == kEmptyKey) return;
        acc[GPF_SUM_COVERED] += 1;
        const unsigned f = (unsigned)(key & 0xffffffffull);
        if (f >= (unsigned)F) {
            bad |= GPF_BAD_INDEX;
            return;
        }
        const double zr = (double)__uint_as_float((unsigned)(key >> 32));
        const double dm = (double)dmap[at];
        const double r = dm - zr;
        const double c0 = c[3 * (size_t)f + 0], c1 = c[3 * (size_t)f + 1], c2 = c[3 * (size_t)f + 2];
        const double m0 = (R00 * c0 + R01 * c1) + R02 * c2, m1 = (R10 * c0 + R11 * c1) + R12 * c2, m2 = (R20 * c0 + R21 * c1) + R22 * c2;
        const double mm = (m0 * m0 + m1 * m1) + m2 * m2;
        if (!(mm < kInf)) {
            bad |= GPF_BAD_INDEX;
            return;
        }
        if (!(dm > 0.0 && dm < kInf && fabs(r) <= gt && mm > 0.0)) return;
        const double b = ((double)py - k5) / k4;
        const double a = (((double)px - k2) - k1 * b) / k0;
        const double q0 = a * zr, q1 = b * zr, q2 = zr;
        const double d0 = r * a, d1 = r * b, d2 = r;
        const double ya = (q0 - t0) / sc, yb = (q1 - t1) / sc, yc = (q2 - t2) / sc;
        const double yy = (ya * ya + yb * yb) + yc * yc;
        double g[6];
        g[0] = yb * m2 - yc * m1, g[1] = yc * m0 - ya * m2, g[2] = ya * m1 - yb * m0, g[3] = m0, g[4] = m1, g[5] = m2;
        const double e = ((m0 * d0 + m1 * d1) + m2 * d2) / sc;
        const double w = 1.0 / mm;
        double h[6];
        bool keep = yy <= GPF_TERM_MAX;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            h[i] = w * g[i];
            keep = keep && (h[i] * g[i] <= GPF_TERM_MAX);
        }
        const double ee = (w * e) * e;
        keep = keep && (ee <= GPF_TERM_MAX);
        if (!keep) {
            bad |= GPF_RANGE;
            return;
        }
        acc[GPF_SUM_COUNT] += 1;
        int o = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) acc[o++] += quantise(h[i] * g[j]);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[GPF_SUM_RHS + i] += quantise(h[i] * e);
        acc[GPF_SUM_EE] += quantise(ee);
    });
    wave_totals(acc, part);
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) bad |= __shfl_xor(bad, w, 64);
    if ((tid & 63) == 0) bad_part[tid >> 6] = bad;
    __syncthreads();
    if (tid < GPF_SUMS) {
        // one wave instruction: 32 lanes, one int64 each (lanes 30 and 31 add 0), into the pair's 256-byte row
        if (workgroup_total(part, GPF_SUM_COVERED)) add_to_row(sums, GPF_SUMS, n, tid, tid < kLive ? workgroup_total(part, tid) : 0);
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < kWaves; ++w) bad |= bad_part[w];
            if (bad) atomicOr(status + n, bad);
        }
    }
}

__device__ __forceinline__ void write_pose(const double* src, double* poses, float* poses32, bool both)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (both) poses[i] = src[i];
        poses32[i] = (float)src[i];
    }
}

__global__ __launch_bounds__(kThreads) void update_kernel(const long long* __restrict__ sums, const int* __restrict__ clipped,
                                                          const double* __restrict__ scale, const double* __restrict__ start, int N,
                                                          long long min_points, double min_pivot, double damping, double tol2,
                                                          double* __restrict__ poses, float* __restrict__ poses32, int* __restrict__ state)
{
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const int st = state[n];
    if (st & GPF_STOP) return;
    const long long* S = sums + GPF_SUMS * (size_t)n;
    double* P = poses + 16 * (size_t)n;
    float* P32 = poses32 + 16 * (size_t)n;
    const long long count = S[GPF_SUM_COUNT];
    int stop = 0;
    double x[6], xx = 0.0;
    if (clipped && clipped[n] != 0) stop = GPF_CLIPPED;
    else if (count < min_points) stop = GPF_FEW;
    else {
        double A[6][6], L[6][6], D[6], u[6];
        const double cnt = (double)count, thr = min_pivot * cnt;
        int o = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) A[i][j] = (double)S[o++] * 0x1p-36;
            A[i][i] = A[i][i] + damping * cnt;
            x[i] = (double)S[GPF_SUM_RHS + i] * 0x1p-36;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double p = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                u[k] = L[j][k] * D[k];
                p = p - L[j][k] * u[k];
            }
            if (!(p > thr)) stop = GPF_DEGENERATE;
            D[j] = p;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double s = A[j][i];
#pragma unroll
                for (int k = 0; k < j; ++k) s = s - L[i][k] * u[k];
                L[i][j] = s / p;
            }
        }
        if (!stop) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int k = 0; k < i; ++k) x[i] = x[i] - L[i][k] * x[k];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
#pragma unroll
            for (int i = 5; i >= 0; --i) {
#pragma unroll
                for (int k = i + 1; k < 6; ++k) x[i] = x[i] - L[k][i] * x[k];
            }
            xx = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
            if (!(xx < kInf)) stop = GPF_DEGENERATE;
        }
    }
    if (stop) {
        state[n] = (st & ~GPF_CONVERGED) | stop;
        if (start) write_pose(start + 16 * (size_t)n, P, P32, true);
        return;
    }
    const double a0 = 0.5 * x[0], a1 = 0.5 * x[1], a2 = 0.5 * x[2];
    const double a00 = a0 * a0, a11 = a1 * a1, a22 = a2 * a2, a01 = a0 * a1, a02 = a0 * a2, a12 = a1 * a2;
    const double s = (a00 + a11) + a22, p = 1.0 - s, q = 1.0 + s;
    double Q[3][3];
    Q[0][0] = (p + 2.0 * a00) / q, Q[0][1] = (2.0 * a01 - 2.0 * a2) / q, Q[0][2] = (2.0 * a02 + 2.0 * a1) / q;
    Q[1][0] = (2.0 * a01 + 2.0 * a2) / q, Q[1][1] = (p + 2.0 * a11) / q, Q[1][2] = (2.0 * a12 - 2.0 * a0) / q;
    Q[2][0] = (2.0 * a02 - 2.0 * a1) / q, Q[2][1] = (2.0 * a12 + 2.0 * a0) / q, Q[2][2] = (p + 2.0 * a22) / q;
    double out[16];
    const double sc = scale[n];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (Q[i][0] * P[j] + Q[i][1] * P[4 + j]) + Q[i][2] * P[8 + j];
        out[4 * i + 3] = P[4 * i + 3] + sc * x[3 + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) out[12 + j] = P[12 + j];
    state[n] = (st & ~GPF_CONVERGED) | (xx < tol2 ? GPF_CONVERGED : 0);
    write_pose(out, P, P32, true);
}

}  // namespace

extern "C" {

int gpf_abi_version(void) { return 1; }

int gpf_pixels_per_workgroup(void) { return kChunk; }

int gpf_face_normals(const float* vertices, int V, const int* faces, int F, double* c, void* stream)
{
    GPF_REQUIRE(V >= 1 && F >= 0, "gpf_face_normals: bad sizes (V >= 1, F >= 0)");
    if (F == 0) return GPF_OK;
    GPF_REQUIRE(vertices && faces && c, "gpf_face_normals: null pointer");
    hipLaunchKernelGGL(face_normals_kernel, dim3((unsigned)(((long long)F + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, vertices, V, faces, F, c);
    GPF_CHECK_LAUNCH("gpf_face_normals");
    return GPF_OK;
}

int gpf_accumulate(const unsigned long long* vis, const double* c, int F, const double* poses, const double* K, const float* depth,
                   int M, const int* frame, const int* box, const double* gate, const double* scale, int N, int H, int W,
                   long long* sums, int* status, void* stream)
{
    GPF_REQUIRE(N >= 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W <= kMaxPixels && F >= 0 && M >= 1,
                "gpf_accumulate: bad sizes (0 <= N <= 65535, H, W > 0, H*W <= 2^22, F >= 0, M >= 1)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && (c || F == 0) && poses && K && depth && frame && box && gate && scale && sums && status,
                "gpf_accumulate: null pointer");
    GPF_REQUIRE(((uintptr_t)sums & 7) == 0 && ((uintptr_t)vis & 7) == 0, "gpf_accumulate: vis or sums is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpf_accumulate", hipMemsetAsync(sums, 0, (size_t)N * GPF_SUMS * sizeof(long long), s));
    GPF_CHECK_HIP("gpf_accumulate", hipMemsetAsync(status, 0, (size_t)N * sizeof(int), s));
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)(((long long)H * W + kChunk - 1) / kChunk), N), dim3(kThreads), 0, s, vis, c, F,
                       poses, K, depth, M, frame, box, gate, scale, H, W, sums, status);
    GPF_CHECK_LAUNCH("gpf_accumulate");
    return GPF_OK;
}

int gpf_update(const long long* sums, const int* clipped, const double* scale, const double* start, int N, long long min_points,
               double min_pivot, double damping, double tol2, double* poses, float* poses32, int* state, void* stream)
{
    GPF_REQUIRE(N >= 0 && N <= 65535, "gpf_update: bad sizes (0 <= N <= 65535)");
    GPF_REQUIRE(min_points >= 0 && min_pivot >= 0.0 && min_pivot < kInf && damping >= 0.0 && damping < kInf && tol2 >= 0.0,
                "gpf_update: min_points, min_pivot, damping and tol2 must be >= 0, min_pivot and damping finite");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(sums && scale && poses && poses32 && state, "gpf_update: null pointer");
    GPF_REQUIRE(((uintptr_t)sums & 7) == 0, "gpf_update: sums is not 8-byte aligned");
    hipLaunchKernelGGL(update_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, sums, clipped,
                       scale, start, N, min_points, min_pivot, damping, tol2, poses, poses32, state);
    GPF_CHECK_LAUNCH("gpf_update");
    return GPF_OK;
}

}  // extern "C"
