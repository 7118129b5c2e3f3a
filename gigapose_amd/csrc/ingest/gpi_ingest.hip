// libgigapose_ingest.so (C-ABI: include/gigapose_ingest.h): the stage BEFORE the hot path -- camera frames (u8) and CNOS
// detections whose masks are still run-length lists go to the GPU as they are; the masks are decoded while the crop is taken.
//   reference: GigaPoseTestSet.add_detections / collate_fn   src/dataloader/test.py:205-318   (rle_to_binary_mask per detection)
//              process_real                                  src/dataloader/train.py:80-123
//              mask_to_rle (the format)                      src/utils/mask.py:9-27
// Format: uncompressed COCO run lengths.  counts = lengths of alternating runs of 0 and 1 over the mask flattened COLUMN-major
// (pixel (y, x) has index p = x*H + y); the first run is zeros and may be empty; the counts sum to H*W.  With cum the inclusive
// prefix sums, pixel p lies in run j = #{i : cum[i] <= p} and its value is j & 1.
// gpi_rle_scan builds cum and validates the list (gp_rle_scan.h, shared with libgigapose_rlestr.so); the fused kernel is the crop
// skeleton of gp_crop_geom.h, shared with gp_crop.hip's preprocess_kernel, over a pixel source that searches cum where the dense
// one reads `masks[d][sy][sx]`, so the two routes agree bit for bit.  The host-side plumbing is gp_front.h's.
// This library links no object of libgigapose_hip.so and exports only gpi_* names.
#include "gigapose_ingest.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpi
#include "../gp_front.h"
#include "../gp_crop_geom.h"
#include "../gp_rle_scan.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kStage = 4096;                        // prefix sums a block stages in LDS (16 KB: 8 blocks per CU keep their 160 KB)

// gpi_rle_scan leaves cum[hi - 1] == H*W on a valid list and -1 on a bad one (negative count or wrong total)
__device__ __forceinline__ bool list_valid(const int* __restrict__ cum, const int* __restrict__ offsets, int d, int total, int HW,
                                           int& lo, int& hi)
{
    return list_range(offsets, d, total, lo, hi) && cum[hi - 1] == HW;
}

// One workgroup per detection: gp_rle_scan.h's scan over the counts as they are.
__global__ __launch_bounds__(kThreads) void rle_scan_kernel(const int* __restrict__ counts, const int* __restrict__ offsets, int total,
                                                            int HW, int* __restrict__ cum, int* __restrict__ err)
{
    __shared__ long long wave_sum[2][kScanWaves];
    __shared__ int bad_any;
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo, hi;
    if (!list_range(offsets, d, total, lo, hi)) {   // no count at all, or a slice outside the arrays: nothing is written
        if (tid == 0) atomicExch(err, d + 1);
        return;
    }
    if (tid == 0) bad_any = 0;
    CumScan scan;
    for (int base = lo; base < hi; base += kScanChunk) {
        const int i0 = base + tid * kScanItems;
        long long v[kScanItems];
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) v[k] = i0 + k < hi ? counts[i0 + k] : 0;
        scan.chunk(v, i0, hi, HW, cum, wave_sum, lane, wave);
    }
    scan.finish(d, hi, HW, cum, err, &bad_any);
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

// the run-search source: the mask value of pixel p = sx*H + sy is the parity of its rank among the window's prefix sums
struct RunSource {
    const uint8_t* frame;
    const int *runs, *win;   // the window [j0, j0 + m) of the list: staged in LDS, or where it is in global memory
    bool staged;
    int j0, m, H, W;
    size_t plane;
    __device__ __forceinline__ void fetch(int sy, int sx, float (&v)[3], float& mk) const
    {
        const int p = sx * H + sy;
        mk = (float)((j0 + (staged ? rank_in(runs, m, p) : rank_in(win, m, p))) & 1);   // one search for the three channels
        masked_rgb(frame, plane, (size_t)sy * W + sx, mk, v);
    }
};

// grid (target rows, D); block = 256 threads, thread = output column
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
    bool bad = false;
    if (threadIdx.x == 0) {
        img = im_id[d];
        int l, h;
        bad = !list_valid(cum, offsets, d, total, H * W, l, h) || img < 0 || img >= n_img;   // a failed scan: skipped, never searched
        lo = l;
        hi = h;
    }
    if (!crop_block_enter(g, boxes, d, y, H, W, target, bad, M, err)) return;
    // runs that intersect the crop's column span [x0*H, (x0+cw)*H); a list that fits the LDS budget whole needs no narrowing
    int first = lo, last = hi - 1;
    if (last - first > kStage) {
        find_window(cum, lo, hi, g.x0 * H, (g.x0 + g.cw) * H - 1, ends);
        __syncthreads();
        first = ends[0];
        last = ends[1];
    }
    const int m = last - first;
    const int* win = cum + first;
    const bool staged = m <= kStage;
    if (staged) {
        for (int i = threadIdx.x; i < m; i += kThreads) runs[i] = win[i];
        __syncthreads();
    }
    const size_t plane = (size_t)H * W;
    const RunSource src = {rgb + (size_t)img * 3 * plane, runs, win, staged, first - lo, m, H, W, plane};
    crop_row_normalized(g, d, y, target, src, m0, m1, m2, s0, s1, s2, tar_img, tar_mask);
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

bool sizes_ok(int D, int H, int W, int total) { return frame_sizes_ok(D, H, W) && total >= 0 && total < (1 << 30); }

}  // namespace

extern "C" {

int gpi_abi_version(void) { return 1; }

int gpi_rle_scan(const int* counts, const int* offsets, int total, int D, int H, int W, int* cum, int* err_flag, void* stream)
{
    GPF_REQUIRE(sizes_ok(D, H, W, total), "gpi_rle_scan: bad sizes (0 <= D <= 65535, H, W > 0, H*W < 2^31, 0 <= total < 2^30)");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(counts && offsets && cum && err_flag, "gpi_rle_scan: null pointer");
    hipLaunchKernelGGL(rle_scan_kernel, dim3(D), dim3(kThreads), 0, (hipStream_t)stream, counts, offsets, total, H * W, cum, err_flag);
    GPF_CHECK_LAUNCH("gpi_rle_scan");
    return GPF_OK;
}

int gpi_preprocess_detections_rle(const uint8_t* rgb, const int* cum, const int* offsets, int total, const long long* boxes,
                                  const int* im_id, int n_img, int D, int H, int W, int target, const float* mean3_host,
                                  const float* std3_host, float* tar_img, float* tar_mask, float* M, int* err_flag, void* stream)
{
    GPF_REQUIRE(sizes_ok(D, H, W, total) && n_img > 0 && target > 0 && target <= 4096, "gpi_preprocess_detections_rle: bad sizes");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(rgb && cum && offsets && boxes && im_id && mean3_host && std3_host && tar_img && tar_mask && M && err_flag,
                "gpi_preprocess_detections_rle: null pointer");
    hipLaunchKernelGGL(preprocess_rle_kernel, dim3(target, D), dim3(kThreads), 0, (hipStream_t)stream, rgb, cum, offsets, total, boxes,
                       im_id, n_img, H, W, target, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1],
                       std3_host[2], tar_img, tar_mask, M, err_flag);
    GPF_CHECK_LAUNCH("gpi_preprocess_detections_rle");
    return GPF_OK;
}

int gpi_rle_decode(const int* cum, const int* offsets, int total, int D, int H, int W, float* masks, void* stream)
{
    GPF_REQUIRE(sizes_ok(D, H, W, total), "gpi_rle_decode: bad sizes");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(cum && offsets && masks, "gpi_rle_decode: null pointer");
    hipLaunchKernelGGL(rle_decode_kernel, dim3(H, D), dim3(kThreads), 0, (hipStream_t)stream, cum, offsets, total, H, W, masks);
    GPF_CHECK_LAUNCH("gpi_rle_decode");
    return GPF_OK;
}

}  // extern "C"
