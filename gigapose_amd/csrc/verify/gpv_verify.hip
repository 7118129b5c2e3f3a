// libgigapose_verify.so (C-ABI: include/gigapose_verify.h): counting, for every pose hypothesis, how the pixels it draws compare
// with the sensor's depth and with the detection's run-length mask -- what a caller chooses among a detection's hypotheses on.
//   reference: the role of the multi-hypothesis refiners (n_pose_hypotheses: 5, src/megapose/utils/load_model.py:27-45); nothing
//   of them is restated here, the header's definitions are the contract.
// counts_kernel walks the pair's box as gp_key_walk.h states it: grid (chunk of 4096 box pixels, pair); the pair rules are judged
// first (a bad frame or mask sets its bit even for an empty box), then a workgroup whose chunk lies beyond the pair's clamped box
// returns before it reads a key.  A wave's 8-byte key loads and 4-byte depth loads are contiguous within a row.  A thread keeps
// the ten counters of its 16 pixels in registers (nine of them 32-bit: a wave's total is at most 1024), then the header's wave
// and workgroup sums, and one atomic add of int64 per counter that is not 0 per workgroup that saw a covered or a masked pixel.
// The mask value of a pixel is the parity of its rank among the detection's prefix sums: a bisection of the pair's slice per BOX
// pixel (the lanes of a wave share the list but not the pixel index, which moves by H from lane to lane).
// Only integers are merged; no float atomics.  gigapose_testing/verify_ref.py restates the arithmetic in numpy; the two agree bit
// for bit.  The host-side plumbing is gp_front.h's, list_range is gp_rle_scan.h's.  This library links no object of the other
// libraries and exports only gpv_* names.
#include <math.h>

#include "gigapose_verify.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpv
#include "../gp_front.h"
#include "../gp_key_walk.h"

namespace {

constexpr int kClasses = 9;                   // 2 x 4 classes of a covered pixel + uncovered in the mask
constexpr int kLive = 10;                     // + the residual
static_assert(GPV_COUNTS == 16 && GPV_UNCOVERED_IN_MASK == kClasses - 1 && GPV_RESIDUAL == kLive - 1 && 2 * GPV_FRONT + 1 == 7,
              "the layout of a row of counts");

// grid (ceil(H*W / 4096), N).  counts (N,16), status (N): zeroed by the caller
__global__ __launch_bounds__(kThreads) void counts_kernel(const u64* __restrict__ vis, const float* __restrict__ depth, int M,
                                                          const int* __restrict__ frame, const int* __restrict__ cum,
                                                          const int* __restrict__ offsets, int total, int D, const int* __restrict__ det,
                                                          const int* __restrict__ box, const double* __restrict__ tol, int H, int W,
                                                          long long* __restrict__ counts, int* __restrict__ status)
{
    __shared__ long long part[kWaves][kLive];
    const int n = blockIdx.y, tid = threadIdx.x;
    // the pair rules: uniform over the workgroup and over the pair's workgroups, like every return below
    int bad = 0, fr = 0, lo = 0, hi = 0;
    if (depth) {
        fr = frame[n];
        if (fr < 0 || fr >= M) bad |= GPV_BAD_FRAME;
    }
    bool masked = false;
    if (cum) {
        const int d = det[n];
        if (d >= 0) {
            masked = true;
            if (!mask_slice(offsets, d, D, total, cum, H, W, lo, hi)) bad |= GPV_BAD_MASK;
        }
    }
    if (bad) {
        if (tid == 0 && blockIdx.x == 0) atomicOr(status + n, bad);
        return;
    }
    BoxWalk walk;
    if (!walk.open(box, n, H, W)) return;                   // no key has been read
    const double t = tol[n];
    const u64* keys = vis + (size_t)n * H * W;
    const float* dmap = depth ? depth + (size_t)fr * H * W : nullptr;

    int acc[kClasses];
#pragma unroll
    for (int i = 0; i < kClasses; ++i) acc[i] = 0;
    long long residual = 0;
    walk.for_each(W, [&](int px, int py, size_t at) {
        const u64 key = keys[at];
        const int in_mask = masked ? (rank_of(cum, lo, hi, px * H + py) & 1) : 0;   // px*H + py < H*W <= 2^22
        if (key == kEmptyKey) {
            acc[GPV_UNCOVERED_IN_MASK] += in_mask;
            return;
        }
        int cls = GPV_UNMEASURED;
        if (dmap) {
            const double dm = (double)dmap[at];
            if (dm > 0.0 && dm < kInf) {
                const double zr = (double)__uint_as_float((unsigned)(key >> 32));
                const double r = dm - zr, ar = fabs(r);
                if (ar <= t) {
                    cls = GPV_AGREE;
                    const double q = t > 0.0 ? ar / t : 0.0;
                    if (q == q) residual += (long long)rint(q * 0x1p20);
                } else if (r > t) cls = GPV_BEHIND;
                else if (r < -t) cls = GPV_FRONT;
            }
        }
        const int slot = 2 * cls + in_mask;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += (slot == i);
    });
    long long last[1] = {residual};
    wave_totals(acc, part);                                 // widened to 64 bits in LDS
    wave_totals(last, part, GPV_RESIDUAL);
    __syncthreads();
    if (tid < kLive) {
        const long long v = workgroup_total(part, tid);
        // a counter that is not 0 belongs to a workgroup that saw a covered or a masked pixel
        if (v) add_to_row(counts, GPV_COUNTS, n, tid, v);
    }
}

}  // namespace

extern "C" {

int gpv_abi_version(void) { return 1; }

int gpv_pixels_per_workgroup(void) { return kChunk; }

int gpv_counts(const unsigned long long* vis, const float* depth, int M, const int* frame, const int* cum, const int* offsets,
               int total, int D, const int* det, const int* box, const double* tol, int N, int H, int W, long long* counts,
               int* status, void* stream)
{
    GPF_REQUIRE(N >= 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W <= kMaxPixels && (!depth || M >= 1) &&
                    (!cum || (D >= 0 && total >= 0)),
                "gpv_counts: bad sizes (0 <= N <= 65535, H, W > 0, H*W <= 2^22; with depth M >= 1; with masks D >= 0, total >= 0)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && box && tol && counts && status && (!depth || frame) && (!cum || (offsets && det)),
                "gpv_counts: null pointer (frame is required with depth; offsets and det with cum)");
    GPF_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)vis & 7) == 0, "gpv_counts: vis or counts is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpv_counts", hipMemsetAsync(counts, 0, (size_t)N * GPV_COUNTS * sizeof(long long), s));
    GPF_CHECK_HIP("gpv_counts", hipMemsetAsync(status, 0, (size_t)N * sizeof(int), s));
    hipLaunchKernelGGL(counts_kernel, dim3((unsigned)(((long long)H * W + kChunk - 1) / kChunk), N), dim3(kThreads), 0, s, vis, depth, M,
                       frame, cum, offsets, total, D, det, box, tol, H, W, counts, status);
    GPF_CHECK_LAUNCH("gpv_counts");
    return GPF_OK;
}

}  // extern "C"
