// The walk of a workgroup over a pair's box of the render library's 64-bit keys, shared by accumulate_kernel (refine/gpf_refine.hip),
// counts_kernel (verify/gpv_verify.hip) and moments_kernel (maskfit/gpm_maskfit.hip): written ONCE, so the three visit the same
// pixels in the same order, judge a detection's mask slice by the same rule and merge their integer sums the same way.  Header
// only, compiled into each of the three libraries (and, for rank_of's constants and the sums alone, into gtinfo/gpg_gtinfo.hip).
// Grid (chunk of kChunk box pixels, pair).  The box is walked row by row, kThreads consecutive box pixels per step, so a wave's
// 8-byte key loads are contiguous within a row; a thread visits kPix pixels.  What a kernel does per pixel, the order of its pair
// rules and the box test, and which totals it adds to global memory stay in the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "gp_rle_scan.h"

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPix = 16;                      // box pixels of a thread
constexpr int kChunk = kThreads * kPix;       // box pixels of a workgroup
constexpr long long kMaxPixels = 1ll << 22;
constexpr u64 kEmptyKey = ~0ull;
constexpr double kInf = (double)INFINITY;

// #{i in [lo, hi) : cum[i] <= p} for a non-decreasing cum; every index read lies in [lo, hi).  The mask value of pixel (px, py) is
// the parity of rank_of(cum, lo, hi, px * H + py);  px*H + py < H*W <= 2^22
__device__ __forceinline__ int rank_of(const int* __restrict__ cum, int lo, int hi, int p)
{
    int a = lo, b = hi;
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if (cum[mid] <= p) a = mid + 1;
        else b = mid;
    }
    return a - lo;
}

// The rule of a detection's mask, d >= 0: its slice [lo, hi) of cum lies inside the arrays and ends at H*W (a list that the scan
// found bad ends at -1).  Uniform over the workgroups of a pair.
__device__ __forceinline__ bool mask_slice(const int* __restrict__ offsets, int d, int D, int total, const int* __restrict__ cum, int H,
                                           int W, int& lo, int& hi)
{
    return d < D && list_range(offsets, d, total, lo, hi) && cum[hi - 1] == H * W;
}

struct BoxWalk {
    int x0, y0, x1, y1;                       // the pair's box clamped to the frame, inclusive
    int bw, area, first;

    // false: the box is empty, or this workgroup's chunk lies beyond it -- nothing has been read but the box, no key.  Uniform
    // over the workgroup.
    __device__ __forceinline__ bool open(const int* __restrict__ box, int n, int H, int W)
    {
        const int* bx = box + 4 * (size_t)n;
        x0 = max(bx[0], 0), y0 = max(bx[1], 0), x1 = min(bx[2], W - 1), y1 = min(bx[3], H - 1);
        if (x1 < x0 || y1 < y0) return false;
        bw = x1 - x0 + 1, area = bw * (y1 - y0 + 1);        // <= H*W <= 2^22
        first = blockIdx.x * kChunk;                        // < 2^22 + 4096
        return first < area;
    }

    // body(px, py, at) for this thread's pixels of the chunk, at = py * W + px
    template <typename Body>
    __device__ __forceinline__ void for_each(int W, Body&& body) const
    {
        for (int s = 0; s < kPix; ++s) {
            const int idx = first + s * kThreads + (int)threadIdx.x;
            if (idx >= area) break;
            const int row = idx / bw, px = x0 + (idx - row * bw), py = y0 + row;
            body(px, py, (size_t)py * W + px);
        }
    }
};

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// The workgroup's sums, in two halves around ONE barrier of the caller's: wave_totals leaves the total of each v[i] over the
// wave in every lane and, widened to 64 bits, in part[wave][at + i]; after the barrier workgroup_total(part, i) is the sum
// over the workgroup.
template <int kCount, typename T, int kRow>
__device__ __forceinline__ void wave_totals(T (&v)[kCount], long long (&part)[kWaves][kRow], int at = 0)
{
#pragma unroll
    for (int i = 0; i < kCount; ++i) v[i] = wave_sum(v[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kCount; ++i) part[threadIdx.x >> 6][at + i] = v[i];
    }
}

template <int kRow>
__device__ __forceinline__ long long workgroup_total(const long long (&part)[kWaves][kRow], int i)
{
    long long out = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) out += part[w][i];
    return out;
}

// the row of pair n of a table of int64 sums takes the workgroup's total v: one atomic add, the result is not used
__device__ __forceinline__ void add_to_row(long long* __restrict__ rows, int stride, int n, int i, long long v)
{
    atomicAdd(reinterpret_cast<u64*>(rows) + stride * (size_t)n + i, (u64)v);
}

}  // namespace
