// Run lengths -> inclusive prefix sums `cum`, one workgroup of 256 threads per detection, shared by gpi_rle_scan
// (ingest/gpi_ingest.hip) and pass 2 of gps_rle_string_scan (rlestr/gps_rle_strings.hip): written ONCE, so the two libraries
// leave the same bits in cum and mark a bad list the same way.  Header only.
// A chunk is 1024 counts: 4 consecutive counts per thread, an inclusive wave scan of the thread sums (__shfl_up, 6 steps), the
// 4 wave totals through LDS; every thread keeps the running carry in a register.  Sums are 64-bit so that a garbage list cannot
// wrap into a plausible total.
// Barrier scheme: ONE barrier per block scan.  The caller hands block_inclusive the LDS slot of this call and must not hand the
// same slot to the next call: a thread that writes slot A again has passed the barrier of the call on slot B in between, which
// every thread reaches only after its reads of A.  CumScan alternates two slots; a caller with one slot follows the call with
// a barrier of its own.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kScanItems = 4;                       // counts per thread and chunk
constexpr int kScanChunk = kScanThreads * kScanItems;

template <typename T>
__device__ __forceinline__ T wave_inclusive(T v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

// Inclusive scan of `v` over the block's threads plus the running `carry` of the earlier chunks, which it advances by this
// chunk's total.  `slot` holds kScanWaves values (see the barrier scheme above).
template <typename T>
__device__ __forceinline__ T block_inclusive(T v, T& carry, T* slot, int lane, int wave)
{
    T incl = wave_inclusive(v, lane);
    if (lane == 63) slot[wave] = incl;
    __syncthreads();
    incl += carry;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
        const T t = slot[w];
        if (w < wave) incl += t;
        carry += t;
    }
    return incl;
}

// A detection's slice [lo, hi) of the run arrays, taken from `offsets` and checked against the arrays' length: every later
// index is bounded by it, never by what the arrays hold.
__device__ __forceinline__ bool list_range(const int* __restrict__ offsets, int d, int total, int& lo, int& hi)
{
    lo = offsets[d];
    hi = offsets[d + 1];
    return 0 <= lo && lo < hi && hi <= total;
}

// The counts -> cum scan of one detection, chunk by chunk.  A valid list leaves cum[hi - 1] == HW; a bad one (a negative count,
// a prefix sum or a total other than HW) leaves cum[hi - 1] == -1 and d + 1 in *err, and is never searched.
struct CumScan {
    long long carry = 0;
    int bad = 0, buf = 0;

    // v: this thread's counts at list positions i0 .. i0 + 3 (0 at and past hi)
    __device__ __forceinline__ void chunk(long long (&v)[kScanItems], int i0, int hi, int HW, int* __restrict__ cum,
                                          long long (*slots)[kScanWaves], int lane, int wave)
    {
        long long s = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            bad |= v[k] < 0;
            s += v[k];
            v[k] = s;
        }
        const long long before = block_inclusive(s, carry, slots[buf], lane, wave) - s;
        buf ^= 1;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            const long long c = before + v[k];
            bad |= c > HW;
            if (i0 + k < hi) cum[i0 + k] = c > HW ? HW : (int)c;   // clamped: a bad list is marked in finish() and never searched
        }
    }

    // *bad_any: an LDS word the block zeroed before a barrier that every thread has passed
    __device__ __forceinline__ void finish(int d, int hi, int HW, int* __restrict__ cum, int* __restrict__ err, int* bad_any)
    {
        if (bad) *bad_any = 1;
        __syncthreads();
        if (threadIdx.x == 0 && (*bad_any || carry != HW)) {
            cum[hi - 1] = -1;
            atomicExch(err, d + 1);
        }
    }
};

}  // namespace
