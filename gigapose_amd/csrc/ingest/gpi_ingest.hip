// libgigapose_ingest.so (C-ABI: include/gigapose_ingest.h): the stage BEFORE the hot path -- camera frames (u8) and CNOS
// detections whose masks are still run-length lists go to the GPU as they are; the masks are decoded while the crop is taken.
//   reference: GigaPoseTestSet.add_detections / collate_fn   src/dataloader/test.py:205-318   (rle_to_binary_mask per detection)
//              process_real                                  src/dataloader/train.py:80-123
//              mask_to_rle (the format)                      src/utils/mask.py:9-27
// Format: uncompressed COCO run lengths.  counts = lengths of alternating runs of 0 and 1 over the mask flattened COLUMN-major
// (pixel (y, x) has index p = x*H + y); the first run is zeros and may be empty; the counts sum to H*W.  With cum the inclusive
// prefix sums, pixel p lies in run j = #{i : cum[i] <= p} and its value is j & 1.
// gpi_rle_scan builds cum (and validates the list); the fused kernel is gp_crop.hip's preprocess_kernel with `masks[d][sy][sx]`
// replaced by a search of cum.  The source-index arithmetic is shared with it (gp_crop_geom.h), so the two routes agree bit for bit.
// This library links no object of libgigapose_hip.so and exports only gpi_* names.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../gp_crop_geom.h"

#define GPI_OK 0
#define GPI_EINVAL -1
#define GPI_ELAUNCH -2

static thread_local char g_err[512] = "";
static void gpi_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define GPI_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            gpi_set_error(__VA_ARGS__); \
            return GPI_EINVAL;          \
        }                               \
    } while (0)

#define GPI_CHECK_LAUNCH(name)                                                   \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) {                                                  \
            gpi_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return GPI_ELAUNCH;                                                  \
        }                                                                        \
    } while (0)

namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;                       // counts per thread and pass of the scan
constexpr int kScanChunk = kThreads * kScanItems;
constexpr int kStage = 4096;                        // prefix sums a block stages in LDS (16 KB: 8 blocks per CU keep their 160 KB)

// A detection's slice [lo, hi) of the run arrays, taken from `offsets` and checked against the arrays' length: every later
// index is bounded by it, never by what the arrays hold.
__device__ __forceinline__ bool list_range(const int* __restrict__ offsets, int d, int total, int& lo, int& hi)
{
    lo = offsets[d];
    hi = offsets[d + 1];
    return 0 <= lo && lo < hi && hi <= total;
}

// gpi_rle_scan leaves cum[hi - 1] == H*W on a valid list and -1 on a bad one (negative count or wrong total)
__device__ __forceinline__ bool list_valid(const int* __restrict__ cum, const int* __restrict__ offsets, int d, int total, int HW,
                                           int& lo, int& hi)
{
    return list_range(offsets, d, total, lo, hi) && cum[hi - 1] == HW;
}

// One workgroup per detection.  Pass = 1024 counts: 4 consecutive counts per thread, an inclusive wave scan of the thread sums
// (__shfl_up, 6 steps), the 4 wave totals through LDS (two buffers alternate, so a pass costs one barrier); every thread keeps the
// running carry in a register.  Sums are 64-bit so that a garbage list cannot wrap into a plausible total.
__global__ __launch_bounds__(kThreads) void rle_scan_kernel(const int* __restrict__ counts, const int* __restrict__ offsets, int total,
                                                            int HW, int* __restrict__ cum, int* __restrict__ err)
{
    constexpr int kWaves = kThreads / 64;
    __shared__ long long wave_sum[2][kWaves];
    __shared__ int bad_any;
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo, hi;
    if (!list_range(offsets, d, total, lo, hi)) {   // no count at all, or a slice outside the arrays: nothing is written
        if (tid == 0) atomicExch(err, d + 1);
        return;
    }
    if (tid == 0) bad_any = 0;
    int bad = 0, buf = 0;
    long long carry = 0;
    for (int base = lo; base < hi; base += kScanChunk, buf ^= 1) {
        const int i0 = base + tid * kScanItems;
        long long v[kScanItems];
        long long s = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            const int c = i0 + k < hi ? counts[i0 + k] : 0;
            bad |= c < 0;
            s += c;
            v[k] = s;
        }
        long long incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wave_sum[buf][wave] = incl;
        __syncthreads();
        long long before = carry + incl - s;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before += wave_sum[buf][w];
            carry += wave_sum[buf][w];
        }
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            const long long c = before + v[k];
            bad |= c > HW;
            if (i0 + k < hi) cum[i0 + k] = c > HW ? HW : (int)c;   // clamped: a bad list is marked below and never searched
        }
    }
    if (bad) bad_any = 1;
    __syncthreads();
    if (tid == 0 && (bad_any || carry != HW)) {
        cum[hi - 1] = -1;
        atomicExch(err, d + 1);
    }
}

// #{i in [a, b) : cum[i] <= p} + a for a non-decreasing cum, by one whole wave: 64 probes per step, so a list of 150 k runs takes 3
// dependent loads where a per-thread bisection takes 18.  Every lane of the wave must call it with the same arguments.
__device__ __forceinline__ int wave_rank(const int* __restrict__ cum, int a, int b, int p, int lane)
{
    while (a < b) {
        const int len = b - a;
        const int s = (len + 63) >> 6;
        long long probe = (long long)a + (long long)lane * s + (s - 1);
        const int idx = probe < b ? (int)probe : b - 1;
        const int c = __popcll(__ballot(cum[idx] <= p));   // cum is monotone: the true lanes are a prefix
        const long long na = (long long)a + (long long)c * s;
        if (c < 64) {
            const long long nb = na + (s - 1);
            b = nb < b - 1 ? (int)nb : b - 1;
        }
        a = na < b ? (int)na : b;
    }
    return a;
}

// #{i in [0, m) : a[i] <= p}
__device__ __forceinline__ int rank_in(const int* a, int m, int p)
{
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The runs a block has to look at: list entries [j0, j0 + m) decide every pixel p of [pa, pb]; entries before j0 are <= pa, entry
// j0 + m (the run that holds pb) is > pb.  Waves 0 and 1 find the two ends at the same time.
__device__ __forceinline__ void find_window(const int* __restrict__ cum, int lo, int hi, int pa, int pb, int* ends)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2) {
        const int r = wave_rank(cum, lo, hi - 1, wave == 0 ? pa : pb, lane);   // cum[hi - 1] == H*W > p: the last entry decides nothing
        if (lane == 0) ends[wave] = r;
    }
}

// grid (target rows, D); block = 256 threads, thread = output column -- the shape of gp_crop.hip's preprocess_kernel
__global__ __launch_bounds__(kThreads) void preprocess_rle_kernel(const uint8_t* __restrict__ rgb, const int* __restrict__ cum,
                                                                  const int* __restrict__ offsets, int total,
                                                                  const long long* __restrict__ boxes, const int* __restrict__ im_id,
                                                                  int n_img, int H, int W, int target, float m0, float m1, float m2,
                                                                  float s0, float s1, float s2, float* __restrict__ tar_img,
                                                                  float* __restrict__ tar_mask, float* __restrict__ M,
                                                                  int* __restrict__ err)
{
    __shared__ CropGeom g;
    __shared__ int img, lo, hi, ends[2];
    __shared__ int runs[kStage];
    const int d = blockIdx.y, y = blockIdx.x;
    if (threadIdx.x == 0) {
        make_geom(boxes + 4 * d, H, W, target, g);
        img = im_id[d];
        if (img < 0 || img >= n_img) g.bad = 1;
        int l, h;
        if (!list_valid(cum, offsets, d, total, H * W, l, h)) g.bad = 1;   // its scan failed: skipped, never searched
        lo = l;
        hi = h;
        if (y == 0) {
            if (g.bad) atomicExch(err, d + 1);
            else write_M(g, M + 9 * d);
        }
    }
    __syncthreads();
    if (g.bad) return;
    // runs that intersect the crop's column span [x0*H, (x0+cw)*H); a list that fits the LDS budget whole needs no narrowing
    int first = lo, last = hi - 1;
    if (last - first > kStage) {
        find_window(cum, lo, hi, g.x0 * H, (g.x0 + g.cw) * H - 1, ends);
        __syncthreads();
        first = ends[0];
        last = ends[1];
    }
    const int j0 = first - lo, m = last - first;
    const int* win = cum + first;
    const bool staged = m <= kStage;
    if (staged) {
        for (int i = threadIdx.x; i < m; i += kThreads) runs[i] = win[i];
        __syncthreads();
    }
    const int sy = source_y(g, y);
    const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    const size_t plane = (size_t)H * W;
    for (int x = threadIdx.x; x < target; x += blockDim.x) {
        const int sx = sy < 0 ? -1 : source_x(g, x);
        float mk = 0.f;
        float v[3] = {0.f, 0.f, 0.f};
        if (sx >= 0) {
            const int p = sx * H + sy;
            const int j = j0 + (staged ? rank_in(runs, m, p) : rank_in(win, m, p));   // one search for the three channels
            mk = (float)(j & 1);
            const size_t o = (size_t)sy * W + sx;
#pragma unroll
            for (int c = 0; c < 3; ++c)  // rgb / 255.0 * mask (train.py:83,107)
                v[c] = ((float)rgb[((size_t)img * 3 + c) * plane + o] / 255.0f) * mk;
        }
        const size_t po = (size_t)y * target + x, tt = (size_t)target * target;
#pragma unroll
        for (int c = 0; c < 3; ++c)  // torchvision Normalize: (x - mean) / std
            tar_img[((size_t)d * 3 + c) * tt + po] = (v[c] - mean[c]) / stdv[c];
        tar_mask[(size_t)d * tt + po] = mk;
    }
}

// grid (H, D): a block writes one mask row, threads along x (coalesced stores); pixel (y, x) searches the whole list
__global__ __launch_bounds__(kThreads) void rle_decode_kernel(const int* __restrict__ cum, const int* __restrict__ offsets, int total, int H,
                                                              int W, float* __restrict__ masks)
{
    __shared__ int runs[kStage];
    const int d = blockIdx.y, y = blockIdx.x;
    int lo, hi;
    if (!list_valid(cum, offsets, d, total, H * W, lo, hi)) return;   // uniform over the block
    const int m = hi - 1 - lo;
    const int* win = cum + lo;
    const bool staged = m <= kStage;
    if (staged) {
        for (int i = threadIdx.x; i < m; i += kThreads) runs[i] = win[i];
        __syncthreads();
    }
    float* row = masks + ((size_t)d * H + y) * W;
    for (int x = threadIdx.x; x < W; x += kThreads) {
        const int p = x * H + y;
        row[x] = (float)((staged ? rank_in(runs, m, p) : rank_in(win, m, p)) & 1);
    }
}

bool sizes_ok(int D, int H, int W, int total)
{
    return D >= 0 && D <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) && total >= 0 && total < (1 << 30);
}

}  // namespace

extern "C" {

int gpi_abi_version(void) { return 1; }
const char* gpi_last_error(void) { return g_err; }

int gpi_rle_scan(const int* counts, const int* offsets, int total, int D, int H, int W, int* cum, int* err_flag, void* stream)
{
    GPI_REQUIRE(sizes_ok(D, H, W, total), "gpi_rle_scan: bad sizes (0 <= D <= 65535, H, W > 0, H*W < 2^31, 0 <= total < 2^30)");
    if (D == 0) return GPI_OK;
    GPI_REQUIRE(counts && offsets && cum && err_flag, "gpi_rle_scan: null pointer");
    hipLaunchKernelGGL(rle_scan_kernel, dim3(D), dim3(kThreads), 0, (hipStream_t)stream, counts, offsets, total, H * W, cum, err_flag);
    GPI_CHECK_LAUNCH("gpi_rle_scan");
    return GPI_OK;
}

int gpi_preprocess_detections_rle(const uint8_t* rgb, const int* cum, const int* offsets, int total, const long long* boxes,
                                  const int* im_id, int n_img, int D, int H, int W, int target, const float* mean3_host,
                                  const float* std3_host, float* tar_img, float* tar_mask, float* M, int* err_flag, void* stream)
{
    GPI_REQUIRE(sizes_ok(D, H, W, total) && n_img > 0 && target > 0 && target <= 4096, "gpi_preprocess_detections_rle: bad sizes");
    if (D == 0) return GPI_OK;
    GPI_REQUIRE(rgb && cum && offsets && boxes && im_id && mean3_host && std3_host && tar_img && tar_mask && M && err_flag,
                "gpi_preprocess_detections_rle: null pointer");
    hipLaunchKernelGGL(preprocess_rle_kernel, dim3(target, D), dim3(kThreads), 0, (hipStream_t)stream, rgb, cum, offsets, total, boxes,
                       im_id, n_img, H, W, target, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1],
                       std3_host[2], tar_img, tar_mask, M, err_flag);
    GPI_CHECK_LAUNCH("gpi_preprocess_detections_rle");
    return GPI_OK;
}

int gpi_rle_decode(const int* cum, const int* offsets, int total, int D, int H, int W, float* masks, void* stream)
{
    GPI_REQUIRE(sizes_ok(D, H, W, total), "gpi_rle_decode: bad sizes");
    if (D == 0) return GPI_OK;
    GPI_REQUIRE(cum && offsets && masks, "gpi_rle_decode: null pointer");
    hipLaunchKernelGGL(rle_decode_kernel, dim3(H, D), dim3(kThreads), 0, (hipStream_t)stream, cum, offsets, total, H, W, masks);
    GPI_CHECK_LAUNCH("gpi_rle_decode");
    return GPI_OK;
}

}  // extern "C"
