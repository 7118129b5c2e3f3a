// libgigapose_maskfit.so (C-ABI: include/gigapose_maskfit.h): fitting a coarse pose to the detection's run-length mask by the
// moments of order 0, 1 and 2 of the two silhouettes -- the in-plane angle, the scale (t_z) and the 2-D translation, the four
// degrees of freedom a silhouette holds.  The reference has no such stage; the header's definitions are the contract.
// mask_moments_kernel: one workgroup per detection, the runs of ones strided over its threads, every run summed in closed form
// (head segment, full columns, tail segment): no pixel is visited.
// moments_kernel walks the pair's box as gp_key_walk.h states it: grid (chunk of 4096 box pixels, pair); the pair rules are judged
// first (a missing or bad mask sets its bit even for an empty box), then a workgroup whose chunk lies beyond the pair's clamped
// box returns before it reads a key.  A thread keeps the eight counters of its 16 pixels in registers, then the header's wave and
// workgroup sums, and one atomic add of int64 per counter that is not 0 per workgroup that saw a covered pixel.  The mask value
// of a COVERED pixel is the parity of its rank among the detection's prefix sums: a bisection of the pair's slice.
// update_kernel: one thread per pair -- the exact integer comparison of two intersections over union, the shape values, the
// rational turn, Heron's step for the scale, the shift; the new pose as f64 and f32.  No square root, no transcendental.
// Only integers are merged; no float atomics.  gigapose_testing/maskfit_ref.py restates the arithmetic; the two agree bit for
// bit.  The host-side plumbing is gp_front.h's, list_range is gp_rle_scan.h's.  This library links no object of the other
// libraries and exports only gpm_* names.
#include <math.h>

#include "gigapose_maskfit.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpm
#include "../gp_front.h"
#include "../gp_key_walk.h"

namespace {

constexpr int kLive = 8;                      // the counters of a pair's row that are written
constexpr int kMoments = 6;                   // n, sum x, y, xx, xy, yy
constexpr int kMaxSide = 16384;
static_assert(GPM_ROW == 16 && GPM_MASK_ROW == kLive && GPM_INTER == kMoments && GPM_EDGE == kLive - 1, "the layout of a row of moments");

__device__ __forceinline__ long long s1(long long m) { return m * (m + 1) / 2; }                 // 0 + 1 + .. + m;  0 for m = -1
__device__ __forceinline__ long long s2(long long m) { return m * (m + 1) * (2 * m + 1) / 6; }   // 0 + 1 + 4 + .. + m*m;  0 for m = -1

// the pixels (x, y0 .. y1) of one column
__device__ __forceinline__ void add_segment(long long (&v)[kMoments], long long x, long long y0, long long y1)
{
    const long long n = y1 - y0 + 1, sy = s1(y1) - s1(y0 - 1), syy = s2(y1) - s2(y0 - 1);
    v[0] += n;
    v[1] += x * n;
    v[2] += sy;
    v[3] += x * x * n;
    v[4] += x * sy;
    v[5] += syy;
}

// the full columns x0 .. x1
__device__ __forceinline__ void add_columns(long long (&v)[kMoments], long long x0, long long x1, long long H)
{
    const long long c = x1 - x0 + 1, sx = s1(x1) - s1(x0 - 1), sxx = s2(x1) - s2(x0 - 1);
    v[0] += c * H;
    v[1] += H * sx;
    v[2] += c * s1(H - 1);
    v[3] += H * sxx;
    v[4] += sx * s1(H - 1);
    v[5] += c * s2(H - 1);
}

// grid (D).  mm (D,8), mstatus (D): every entry is written
__global__ __launch_bounds__(kThreads) void mask_moments_kernel(const int* __restrict__ cum, const int* __restrict__ offsets, int total,
                                                                int H, int W, long long* __restrict__ mm, int* __restrict__ mstatus)
{
    __shared__ long long part[kWaves][kLive];
    const int d = blockIdx.x, tid = threadIdx.x;
    int lo, hi;
    const bool good = mask_slice(offsets, d, (int)gridDim.x, total, cum, H, W, lo, hi);  // uniform over the workgroup
    if (tid == 0) mstatus[d] = good ? 0 : GPM_BAD_MASK;
    if (!good) {
        if (tid < GPM_MASK_ROW) mm[GPM_MASK_ROW * (size_t)d + tid] = 0;
        return;
    }
    long long v[kMoments];
#pragma unroll
    for (int i = 0; i < kMoments; ++i) v[i] = 0;
    const long long HW = (long long)H * W;
    for (long long i = (long long)lo + 1 + 2 * tid; i < hi; i += 2 * kThreads) {        // the runs of ones; lo <= i - 1, i < hi <= total
        const long long a = cum[i - 1], b = cum[i];
        if (!(0 <= a && a < b && b <= HW)) continue;
        const long long xa = a / H, ya = a % H, xb = (b - 1) / H, yb = (b - 1) % H;
        if (xa == xb) {
            add_segment(v, xa, ya, yb);
            continue;
        }
        add_segment(v, xa, ya, H - 1);
        add_segment(v, xb, 0, yb);
        if (xb - xa >= 2) add_columns(v, xa + 1, xb - 1, H);
    }
    wave_totals(v, part);
    __syncthreads();
    if (tid < GPM_MASK_ROW) mm[GPM_MASK_ROW * (size_t)d + tid] = tid < kMoments ? workgroup_total(part, tid) : 0;
}

// grid (ceil(H*W / 4096), N).  rows (N,16), status (N): zeroed by the caller
__global__ __launch_bounds__(kThreads) void moments_kernel(const u64* __restrict__ vis, const int* __restrict__ cum,
                                                           const int* __restrict__ offsets, int total, int D, const int* __restrict__ det,
                                                           const int* __restrict__ box, int H, int W, long long* __restrict__ rows,
                                                           int* __restrict__ status)
{
    __shared__ long long part[kWaves][kLive];
    const int n = blockIdx.y, tid = threadIdx.x;
    // the pair rules: uniform over the workgroup and over the pair's workgroups, like every return below
    int bad = 0, lo = 0, hi = 0;
    const int d = det[n];
    if (d < 0) bad = GPM_NO_MASK;
    else if (!mask_slice(offsets, d, D, total, cum, H, W, lo, hi)) bad = GPM_BAD_MASK;
    if (bad) {
        if (tid == 0 && blockIdx.x == 0) atomicOr(status + n, bad);
        return;
    }
    BoxWalk walk;
    if (!walk.open(box, n, H, W)) return;                   // no key has been read
    const int x0 = walk.x0, y0 = walk.y0, x1 = walk.x1, y1 = walk.y1;
    const bool ex0 = x0 > 0, ey0 = y0 > 0, ex1 = x1 < W - 1, ey1 = y1 < H - 1;   // the box's edges that are not the frame's
    const u64* keys = vis + (size_t)n * H * W;

    long long v[kLive];
#pragma unroll
    for (int i = 0; i < kLive; ++i) v[i] = 0;
    walk.for_each(W, [&](int px, int py, size_t at) {
        if (keys[at] == kEmptyKey) return;
        const long long x = px, y = py;                     // < 16384: a product below 2^28
        v[0] += 1;
        v[1] += x;
        v[2] += y;
        v[3] += x * x;
        v[4] += x * y;
        v[5] += y * y;
        v[GPM_INTER] += rank_of(cum, lo, hi, px * H + py) & 1;                  // px*H + py < H*W <= 2^22
        v[GPM_EDGE] += ((px == x0 && ex0) || (px == x1 && ex1) || (py == y0 && ey0) || (py == y1 && ey1)) ? 1 : 0;
    });
    wave_totals(v, part);
    __syncthreads();
    if (tid < kLive) {
        const long long sum = workgroup_total(part, tid);
        // a counter that is not 0 belongs to a workgroup that saw a covered pixel
        if (sum) add_to_row(rows, GPM_ROW, n, tid, sum);
    }
}

struct Shape {
    double mx, my, a, b, tr;
};

__device__ __forceinline__ Shape shape_values(const long long* __restrict__ S)
{
    const double n = (double)S[0];
    Shape v;
    v.mx = (double)S[1] / n;
    v.my = (double)S[2] / n;
    const double uxx = (double)S[3] / n - v.mx * v.mx;
    const double uxy = (double)S[4] / n - v.mx * v.my;
    const double uyy = (double)S[5] / n - v.my * v.my;
    v.a = uxx - uyy;
    v.b = 2.0 * uxy;
    v.tr = uxx + uyy;
    return v;
}

__device__ __forceinline__ void store_pose(double* __restrict__ P, float* __restrict__ P32, const double* __restrict__ src)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double x = src[i];
        P[i] = x;
        P32[i] = (float)x;
    }
}

// grid (ceil(N / 256)): one thread per pair
__global__ __launch_bounds__(kThreads) void update_kernel(const long long* __restrict__ rows, const int* __restrict__ status,
                                                          const long long* __restrict__ mm, int D, const int* __restrict__ det,
                                                          const int* __restrict__ clipped, const double* __restrict__ K,
                                                          const double* __restrict__ start, int N, int it, int last, long long min_points,
                                                          double min_elongation, double gain, double* __restrict__ poses,
                                                          float* __restrict__ poses32, double* __restrict__ best,
                                                          long long* __restrict__ score, int* __restrict__ state)
{
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    double* P = poses + 16 * (size_t)n;
    float* P32 = poses32 + 16 * (size_t)n;
    double* B = best + 16 * (size_t)n;
    long long* sc = score + 4 * (size_t)n;
    int* st = state + 2 * (size_t)n;
    if (it == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) B[i] = P[i];
        sc[0] = 0, sc[1] = 1, sc[2] = 0, sc[3] = 1;
        st[0] = 0, st[1] = 0;
    }
    const int bits = st[0];
    if (bits & GPM_STOP) return;
    const int d = det[n];
    int stop = status[n] & (GPM_BAD_MASK | GPM_NO_MASK);
    if (!stop && (d < 0 || d >= D)) stop = d < 0 ? GPM_NO_MASK : GPM_BAD_MASK;
    if (clipped && clipped[n] != 0) stop |= GPM_CLIPPED;
    const long long* SD = rows + GPM_ROW * (size_t)n;
    const long long* SM = mm + GPM_MASK_ROW * (size_t)(stop ? 0 : d);   // read only where d is in [0, D)
    if (!stop && (SD[0] < min_points || SM[0] < min_points)) stop = GPM_FEW;
    if (stop) {
        st[0] = (bits & ~GPM_ROUND) | stop | GPM_NOT_IMPROVED;
        st[1] = 0;
        sc[0] = sc[2], sc[1] = sc[3];
        const double* S0 = start + 16 * (size_t)n;
#pragma unroll
        for (int i = 0; i < 16; ++i) B[i] = S0[i];
        store_pose(P, P32, S0);
        return;
    }
    const long long inter = SD[GPM_INTER], uni = SD[0] + SM[0] - inter;
    if (it == 0) {
        sc[0] = inter, sc[1] = uni, sc[2] = inter, sc[3] = uni;
    } else if (SD[GPM_EDGE] == 0 && inter * sc[1] > sc[0] * uni) {
#pragma unroll
        for (int i = 0; i < 16; ++i) B[i] = P[i];
        sc[0] = inter, sc[1] = uni;
        st[1] = it;
    }
    if (last) {
        store_pose(P, P32, B);
        if (st[1] == 0) st[0] = bits | GPM_NOT_IMPROVED;
        return;
    }
    const Shape sd = shape_values(SD), sm = shape_values(SM);
    const double e2 = min_elongation * min_elongation;
    const double dot = sd.a * sm.a + sd.b * sm.b;
    const double cross = sd.a * sm.b - sd.b * sm.a;
    const bool turned = sd.a * sd.a + sd.b * sd.b >= e2 * (sd.tr * sd.tr) && sm.a * sm.a + sm.b * sm.b >= e2 * (sm.tr * sm.tr) && dot > 0.0 &&
                        fabs(cross) <= dot;
    const double tau = turned ? (gain * (cross / dot)) / 4.0 : 0.0;
    const double tt = tau * tau, den = 1.0 + tt;
    const double c = (1.0 - tt) / den, s = (2.0 * tau) / den;
    double Q[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        Q[j] = c * P[j] - s * P[4 + j];
        Q[4 + j] = s * P[j] + c * P[4 + j];
        Q[8 + j] = P[8 + j];
        Q[12 + j] = P[12 + j];
    }
    double g = (1.0 + (double)SD[0] / (double)SM[0]) / 2.0;
    g = 1.0 + gain * (g - 1.0);
    if (g < 0.5) g = 0.5;
    if (g > 2.0) g = 2.0;
    const double* k = K + 9 * (size_t)n;
    double t0 = Q[3], t1 = Q[7], t2 = Q[11];
    const double ox = ((k[0] * t0 + k[1] * t1) + k[2] * t2) / t2;
    const double oy = ((k[3] * t0 + k[4] * t1) + k[5] * t2) / t2;
    const double dx = sd.mx - k[2], dy = sd.my - k[5];
    const double px = k[2] + (c * dx - s * dy), py = k[5] + (s * dx + c * dy);
    const double qx = ox + (px - ox) / g, qy = oy + (py - oy) / g;
    t0 = g * t0, t1 = g * t1, t2 = g * t2;
    Q[3] = t0 + ((gain * (sm.mx - qx)) * t2) / k[0];
    Q[7] = t1 + ((gain * (sm.my - qy)) * t2) / k[4];
    Q[11] = t2;
    store_pose(P, P32, Q);
    st[0] = (bits & ~GPM_ROUND) | (turned ? 0 : GPM_ROUND);
}

bool mask_sizes_ok(int total, int D, int H, int W)
{
    return D >= 0 && total >= 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && (long long)H * W <= kMaxPixels;
}

}  // namespace

extern "C" {

int gpm_abi_version(void) { return 1; }

int gpm_pixels_per_workgroup(void) { return kChunk; }

int gpm_mask_moments(const int* cum, const int* offsets, int total, int D, int H, int W, long long* mm, int* mstatus, void* stream)
{
    GPF_REQUIRE(mask_sizes_ok(total, D, H, W), "gpm_mask_moments: bad sizes (D >= 0, total >= 0, 0 < H, W <= 16384, H*W <= 2^22)");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(cum && offsets && mm && mstatus, "gpm_mask_moments: null pointer");
    GPF_REQUIRE(((uintptr_t)mm & 7) == 0, "gpm_mask_moments: mm is not 8-byte aligned");
    hipLaunchKernelGGL(mask_moments_kernel, dim3((unsigned)D), dim3(kThreads), 0, (hipStream_t)stream, cum, offsets, total, H, W, mm, mstatus);
    GPF_CHECK_LAUNCH("gpm_mask_moments");
    return GPF_OK;
}

int gpm_moments(const unsigned long long* vis, const int* cum, const int* offsets, int total, int D, const int* det, const int* box,
                int N, int H, int W, long long* rows, int* status, void* stream)
{
    GPF_REQUIRE(N >= 0 && N <= 65535 && mask_sizes_ok(total, D, H, W),
                "gpm_moments: bad sizes (0 <= N <= 65535, D >= 0, total >= 0, 0 < H, W <= 16384, H*W <= 2^22)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && cum && offsets && det && box && rows && status, "gpm_moments: null pointer");
    GPF_REQUIRE(((uintptr_t)rows & 7) == 0 && ((uintptr_t)vis & 7) == 0, "gpm_moments: vis or rows is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpm_moments", hipMemsetAsync(rows, 0, (size_t)N * GPM_ROW * sizeof(long long), s));
    GPF_CHECK_HIP("gpm_moments", hipMemsetAsync(status, 0, (size_t)N * sizeof(int), s));
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)(((long long)H * W + kChunk - 1) / kChunk), N), dim3(kThreads), 0, s, vis, cum, offsets,
                       total, D, det, box, H, W, rows, status);
    GPF_CHECK_LAUNCH("gpm_moments");
    return GPF_OK;
}

int gpm_update(const long long* rows, const int* status, const long long* mm, int D, const int* det, const int* clipped, const double* K,
               const double* start, int N, int it, int last, long long min_points, double min_elongation, double gain, double* poses,
               float* poses32, double* best, long long* score, int* state, void* stream)
{
    GPF_REQUIRE(N >= 0 && N <= 65535 && D >= 0 && it >= 0, "gpm_update: bad sizes (0 <= N <= 65535, D >= 0, it >= 0)");
    GPF_REQUIRE(min_points >= 1 && min_elongation >= 0.0 && min_elongation < kInf && gain > 0.0 && gain <= 1.0,
                "gpm_update: min_points must be >= 1, min_elongation finite and >= 0, gain in (0, 1]");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(rows && status && (mm || D == 0) && det && K && start && poses && poses32 && best && score && state, "gpm_update: null pointer");
    GPF_REQUIRE((((uintptr_t)rows | (uintptr_t)mm | (uintptr_t)score) & 7) == 0, "gpm_update: rows, mm or score is not 8-byte aligned");
    hipLaunchKernelGGL(update_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, rows, status, mm,
                       D, det, clipped, K, start, N, it, last, min_points, min_elongation, gain, poses, poses32, best, score, state);
    GPF_CHECK_LAUNCH("gpm_update");
    return GPF_OK;
}

}  // extern "C"
