// libgigapose_rlestr.so (C-ABI: include/gigapose_rlestr.h): COCO COMPRESSED run-length strings (the `counts` of a COCO-results json,
// what pycocotools' mask.encode writes) decoded on the GPU into the run lists and prefix sums libgigapose_ingest.so consumes.
//   reference: rle_to_binary_mask per detection (bop_toolkit's pycoco_utils, called at src/dataloader/test.py:238), on the CPU
// Coding (include/gigapose_rlestr.h has it in full): list position m carries x[m] = counts[m] (m <= 2) or counts[m] - counts[m-2]
// (m >= 3); x is written as little-endian 5-bit groups, one per character c + 48, bit 0x20 = "another group follows", bit 0x10 of
// the last group = sign.  So a token ends at every character whose 0x20 bit is clear, counts[0] stands alone, the even positions
// >= 2 are a running sum of the even x and the odd positions one of the odd x.
// One workgroup per detection, two passes:
//   1. over the bytes: every thread counts the terminators among its 8 bytes, a block scan gives each terminator its list position
//      m, the thread that owns a terminator assembles the token by looking BACK (at most 7 bytes, never before the slice start) and
//      stores x[m] in the detection's slot of `counts`;
//   2. over the tokens: two running sums (one per parity) turn x into counts, a third one counts into cum.
// A detection without bytes is an uncompressed list: only pass 2's third sum runs over it.  That sum is gp_rle_scan.h's, the
// code gpi_rle_scan (csrc/ingest/gpi_ingest.hip) runs, so one launch serves a mixed batch and cum has the same bits either way.
// The host-side plumbing is gp_front.h's.
// This library links no object of the other libraries and exports only gps_* names.
#include "gigapose_rlestr.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gps
#include "../gp_front.h"
#include "../gp_rle_scan.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kWaves = kScanWaves;
constexpr int kByteItems = 8;                       // bytes per thread and chunk of pass 1: one aligned 64-bit load
constexpr int kByteChunk = kThreads * kByteItems;
constexpr int kMaxToken = 7;                        // characters of a value below 2^31 (35 bits)
static_assert(kScanItems % 2 == 0, "pass 2: a thread's first token has even m");

// gp_rle_scan.h's block_inclusive for two sums at once, the even and the odd chain of pass 2, on ONE slot: the second barrier
// lets the next call reuse it.
__device__ __forceinline__ void block_inclusive2(long long& a, long long& b, long long& carry_a, long long& carry_b, long long (*lds)[2],
                                                 int lane, int wave)
{
    a = wave_inclusive(a, lane);
    b = wave_inclusive(b, lane);
    if (lane == 63) {
        lds[wave][0] = a;
        lds[wave][1] = b;
    }
    __syncthreads();
    a += carry_a;
    b += carry_b;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const long long ta = lds[w][0], tb = lds[w][1];
        if (w < wave) {
            a += ta;
            b += tb;
        }
        carry_a += ta;
        carry_b += tb;
    }
    __syncthreads();
}

__device__ __forceinline__ bool char_ok(int c) { return c >= 48 && c <= 111; }

// The token whose LAST character sits at byte p: walk back over the characters that say "another group follows" -- at most
// kMaxToken of them, never before the slice start `ba`, never over a byte outside 48..111 (its owner flags it).  Going from the
// last group to the first, the value is a Horner sum in base 32; the sign comes from bit 0x10 of the last group.
__device__ __forceinline__ long long token_ending_at(const uint8_t* __restrict__ bytes, long long ba, long long p, int last, int& bad)
{
    long long x = (last & 0x1f) - ((last & 0x10) ? 32 : 0);
    int len = 1;
    for (; len <= kMaxToken && p - len >= ba; ++len) {
        const int c = bytes[p - len];
        if (!char_ok(c) || !((c - 48) & 0x20)) break;
        if (len < kMaxToken) x = x * 32 + ((c - 48) & 0x1f);
    }
    bad |= len > kMaxToken;                          // an eighth character of the same token
    return x;
}

__global__ __launch_bounds__(kThreads) void rle_string_scan_kernel(const uint8_t* __restrict__ bytes, const int* __restrict__ byte_offsets,
                                                                   int n_bytes, const int* __restrict__ offsets, int total, int HW,
                                                                   int* counts, int* __restrict__ cum, int* __restrict__ err)
{
    __shared__ long long lds_sum[2][kWaves], lds_pair[kWaves][2];
    __shared__ int lds_cnt[2][kWaves];
    __shared__ int bad_any;
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo, hi;
    if (!list_range(offsets, d, total, lo, hi)) {   // no slot at all, or a slice outside the arrays: nothing is written
        if (tid == 0) atomicExch(err, d + 1);
        return;
    }
    if (tid == 0) bad_any = 0;
    __syncthreads();
    const long long ba = byte_offsets[d], bb = byte_offsets[d + 1];
    const bool is_string = ba != bb;
    int bad = 0;
    if (is_string) {
        if (!(0 <= ba && ba < bb && bb <= n_bytes)) {   // a byte slice outside the array: marked without reading a byte
            if (tid == 0) {
                cum[hi - 1] = -1;
                atomicExch(err, d + 1);
            }
            return;
        }
        // pass 1.  Chunks start on an 8-byte ADDRESS boundary at or before the slice, so that a thread whose 8 bytes lie wholly
        // inside the slice loads them as one word; the threads at the two ends load byte by byte, and only bytes of the slice.
        const long long first = ba - (long long)(((uintptr_t)bytes + (uintptr_t)ba) & 7);
        int n_tokens = 0, buf = 0;                   // carry: terminators in the earlier chunks; the slot of lds_cnt in turn
        for (long long base = first; base < bb; base += kByteChunk, buf ^= 1) {
            const long long p0 = base + (long long)tid * kByteItems;
            unsigned long long w = 0;
            if (p0 >= ba && p0 + kByteItems <= bb) {
                w = *reinterpret_cast<const unsigned long long*>(bytes + p0);
            } else {
#pragma unroll
                for (int k = 0; k < kByteItems; ++k)
                    if (p0 + k >= ba && p0 + k < bb) w |= (unsigned long long)bytes[p0 + k] << (8 * k);
            }
            int ends = 0;                            // bit k: byte k of this thread ends a token
#pragma unroll
            for (int k = 0; k < kByteItems; ++k) {
                if (p0 + k < ba || p0 + k >= bb) continue;
                const int c = (int)((w >> (8 * k)) & 0xff);
                bad |= !char_ok(c);
                const bool more = ((c - 48) & 0x20) != 0;
                if (!more) ends |= 1 << k;
                if (p0 + k == bb - 1) bad |= more;   // the string stops inside a token
            }
            const int mine = __popc(ends);
            int m = block_inclusive(mine, n_tokens, lds_cnt[buf], lane, wave) - mine;
#pragma unroll
            for (int k = 0; k < kByteItems; ++k) {
                if (!(ends & (1 << k))) continue;
                const long long x = token_ending_at(bytes, ba, p0 + k, (int)((w >> (8 * k)) & 0xff) - 48, bad);
                const bool fits = x >= INT32_MIN && x <= INT32_MAX;   // a legal x is a difference of two counts in [0, H*W]
                bad |= !fits;
                if (m < hi - lo) counts[lo + m] = fits ? (int)x : (x < 0 ? INT32_MIN : INT32_MAX);
                ++m;
            }
        }
        bad |= n_tokens != hi - lo;                  // the host counted other terminators than the string holds
        if (bad) bad_any = 1;
        __syncthreads();                             // also: every x is stored before pass 2 loads it
        if (bad_any) {                               // some slots may hold no x: pass 2 has nothing to sum
            if (tid == 0) {
                cum[hi - 1] = -1;
                atomicExch(err, d + 1);
            }
            return;
        }
    }
    // pass 2.  Chunk = 1024 list entries, 4 consecutive ones per thread, the first at an even position.  A string's entries hold x:
    // counts[m] is the running sum of its parity's x (position 0 stands alone, the even chain starts at 2); 64-bit, so that garbage
    // cannot wrap into a plausible value.  A count outside [0, H*W] is bad and stored clamped to [-1, H*W].  Then cum by the
    // scan gpi_rle_scan runs (gp_rle_scan.h): inclusive 64-bit sums, clamped to H*W.
    long long carry_even = 0, carry_odd = 0;
    CumScan scan;
    for (int base = lo; base < hi; base += kScanChunk) {
        const int i0 = base + tid * kScanItems;
        long long v[kScanItems];
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) v[k] = i0 + k < hi ? counts[i0 + k] : 0;
        if (is_string) {
            const long long head = i0 == lo ? v[0] : 0;   // x[0]: not part of the even chain
            const long long se = (v[0] - head) + v[2], so = v[1] + v[3];
            long long even0 = se, odd0 = so;
            block_inclusive2(even0, odd0, carry_even, carry_odd, lds_pair, lane, wave);
            even0 -= se;
            odd0 -= so;
            v[2] = even0 + (v[0] - head) + v[2];
            v[0] = i0 == lo ? head : even0 + v[0];
            v[3] = odd0 + v[1] + v[3];
            v[1] = odd0 + v[1];
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) {
                scan.bad |= i0 + k < hi && (v[k] < 0 || v[k] > HW);
                v[k] = v[k] < 0 ? -1 : (v[k] > HW ? HW : v[k]);
                if (i0 + k < hi) counts[i0 + k] = (int)v[k];
                else v[k] = 0;
            }
        }
        scan.chunk(v, i0, hi, HW, cum, lds_sum, lane, wave);
    }
    scan.finish(d, hi, HW, cum, err, &bad_any);
}

}  // namespace

extern "C" {

int gps_abi_version(void) { return 1; }

int gps_rle_string_scan(const uint8_t* bytes, const int* byte_offsets, int n_bytes, const int* offsets, int total, int D, int H, int W,
                        int* counts, int* cum, int* err_flag, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(D, H, W) && total >= 0 && total < (1 << 30) && n_bytes >= 0,
                "gps_rle_string_scan: bad sizes (0 <= D <= 65535, H, W > 0, H*W < 2^31, 0 <= total < 2^30, 0 <= n_bytes < 2^31)");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(byte_offsets && offsets && counts && cum && err_flag && (bytes || n_bytes == 0), "gps_rle_string_scan: null pointer");
    hipLaunchKernelGGL(rle_string_scan_kernel, dim3(D), dim3(kThreads), 0, (hipStream_t)stream, bytes, byte_offsets, n_bytes, offsets, total,
                       H * W, counts, cum, err_flag);
    GPF_CHECK_LAUNCH("gps_rle_string_scan");
    return GPF_OK;
}

}  // extern "C"
