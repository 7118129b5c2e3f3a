// libgigapose_coco.so (C-ABI: include/gigapose_coco.h): scoring detections -- run-length mask intersections, COCO's greedy
// matching, the suppression bits of a mask-IoU NMS.
//   reference: none -- the reference installs pycocotools for this; the header's definitions are the contract.
// fg_scan_kernel: grid (mask), 256 threads; chunks of 1024 runs, 4 consecutive runs per thread, the block scan of gp_rle_scan.h
// on two alternating LDS slots.  mask_inter_kernel: a wave per pair, 4 pairs per workgroup; the lanes stride the odd runs of the
// mask with fewer runs and search the other one twice per run; a butterfly sums.  box_inter_kernel: a thread per pair.
// match_kernel: grid (group, threshold), one wave; lane l holds the ground truths l, l + 64, .. and their matched bits in one
// 64-bit register; detections in order, the best candidate by a butterfly under a total order.  sup_bits_kernel: a wave per (row,
// word), one __ballot.
// Only integers, no division, no atomics: nothing depends on launch geometry.  gigapose_testing/coco_ref.py restates the
// arithmetic; the two agree bit for bit.  The host-side plumbing is gp_front.h's, list_range and block_inclusive gp_rle_scan.h's.
// This library links no object of the other libraries and exports only gpc_* names.
#include "gigapose_coco.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpc
#include "../gp_front.h"
#include "../gp_rle_scan.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kThreads == kScanThreads && GPC_MAX_GROUP_GT == 64 * 64, "the shapes below");

// ------------------------------------------------------------------------------------------------ foreground prefix sums
// grid (D)
__global__ __launch_bounds__(kThreads) void fg_scan_kernel(const int* __restrict__ cum, const int* __restrict__ offsets, int total, int HW,
                                                           int* __restrict__ fg, i64* __restrict__ area, int* __restrict__ status)
{
    __shared__ i64 slots[2][kScanWaves];
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo, hi;
    if (!list_range(offsets, d, total, lo, hi) || cum[hi - 1] != HW) {  // uniform over the workgroup
        if (tid == 0) area[d] = 0, status[d] = GPC_BAD_MASK;
        return;
    }
    i64 carry = 0;
    int buf = 0;
    for (i64 base = lo; base < hi; base += kScanChunk) {              // the same trips in every thread: one barrier each
        const i64 i0 = base + (i64)kScanItems * tid;
        i64 v[kScanItems], s = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            const i64 i = i0 + k;
            if (i < hi && ((i - lo) & 1)) s += (i64)cum[i] - (i64)cum[i - 1];     // an odd run: lo < i < hi <= total
            v[k] = s;
        }
        const i64 before = block_inclusive(s, carry, slots[buf], lane, wave) - s;
        buf ^= 1;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k)
            if (i0 + k < hi) fg[i0 + k] = (int)(before + v[k]);
    }
    if (tid == 0) area[d] = carry, status[d] = 0;
}

// ------------------------------------------------------------------------------------------------ mask intersections
// F_M(x) of the header for the slice [lo, lo + n) of (cum, fg)
__device__ __forceinline__ i64 fg_below(const int* __restrict__ cum, const int* __restrict__ fg, int lo, int n, int x)
{
    int a = 0, b = n;                                                 // the first j in [0, n) with cum[lo + j] > x, n if none
    while (a < b) {
        const int m = a + ((b - a) >> 1);                             // a <= m < b <= n: lo + m < hi
        if (cum[lo + m] > x) b = m;
        else a = m + 1;
    }
    i64 f = a > 0 ? (i64)fg[lo + a - 1] : 0;
    if (a < n && (a & 1)) f += (i64)x - (i64)cum[lo + a - 1];         // a odd: a >= 1
    return f;
}

__device__ __forceinline__ i64 wave_sum(i64 v)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// grid (ceil(P / 4))
__global__ __launch_bounds__(kThreads) void mask_inter_kernel(const int* __restrict__ cumA, const int* __restrict__ offA, const int* __restrict__ fgA,
                                                              int totalA, int DA, const int* __restrict__ cumB, const int* __restrict__ offB,
                                                              const int* __restrict__ fgB, int totalB, int DB, int HW, const int* __restrict__ pair_a,
                                                              const int* __restrict__ pair_b, int P, i64* __restrict__ inter, int* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kWaves + ((int)threadIdx.x >> 6);      // < 65535 + 4
    if (p >= P) return;                                               // the whole wave: no barrier below
    const int a = pair_a[p], b = pair_b[p];
    int flag = 0, loA = 0, hiA = 0, loB = 0, hiB = 0;
    if (a < 0 || a >= DA || b < 0 || b >= DB) flag = GPC_PAIR_RANGE;
    else if (!list_range(offA, a, totalA, loA, hiA) || cumA[hiA - 1] != HW || !list_range(offB, b, totalB, loB, hiB) || cumB[hiB - 1] != HW)
        flag = GPC_PAIR_MASK;
    i64 sum = 0;
    if (!flag) {                                                      // uniform over the wave
        const bool walk_a = hiA - loA <= hiB - loB;
        const int* wc = walk_a ? cumA : cumB;
        const int wlo = walk_a ? loA : loB, wn = walk_a ? hiA - loA : hiB - loB;
        const int* sc = walk_a ? cumB : cumA;
        const int* sf = walk_a ? fgB : fgA;
        const int slo = walk_a ? loB : loA, sn = walk_a ? hiB - loB : hiA - loA;
        for (i64 i = 1 + 2 * (i64)lane; i < wn; i += 128)              // 1 <= i < wn: wlo + i - 1 >= wlo, wlo + i < its hi
            sum += fg_below(sc, sf, slo, sn, wc[wlo + i]) - fg_below(sc, sf, slo, sn, wc[wlo + i - 1]);
        sum = wave_sum(sum);
    }
    if (lane == 0) inter[p] = sum, status[p] = flag;
}

// ------------------------------------------------------------------------------------------------ box intersections
__device__ __forceinline__ int clamp_coord(int v) { return min(max(v, -GPC_MAX_COORD), GPC_MAX_COORD); }

__device__ __forceinline__ i64 box_area(int x0, int y0, int x1, int y1)
{
    return (i64)max(0, x1 - x0) * (i64)max(0, y1 - y0);               // each factor <= 2^22
}

// grid (ceil(P / 256))
__global__ __launch_bounds__(kThreads) void box_inter_kernel(const int* __restrict__ boxA, int DA, const int* __restrict__ boxB, int DB,
                                                             const int* __restrict__ pair_a, const int* __restrict__ pair_b, int P,
                                                             i64* __restrict__ inter, i64* __restrict__ area_a, i64* __restrict__ area_b,
                                                             int* __restrict__ status)
{
    const int p = blockIdx.x * kThreads + (int)threadIdx.x;           // < 65535 + 256
    if (p >= P) return;
    const int a = pair_a[p], b = pair_b[p];
    if (a < 0 || a >= DA || b < 0 || b >= DB) {
        inter[p] = 0, area_a[p] = 0, area_b[p] = 0, status[p] = GPC_PAIR_RANGE;
        return;
    }
    int A[4], B[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) A[i] = clamp_coord(boxA[4 * (size_t)a + i]), B[i] = clamp_coord(boxB[4 * (size_t)b + i]);
    inter[p] = box_area(max(A[0], B[0]), max(A[1], B[1]), min(A[2], B[2]), min(A[3], B[3]));
    area_a[p] = box_area(A[0], A[1], A[2], A[3]);
    area_b[p] = box_area(B[0], B[1], B[2], B[3]);
    status[p] = 0;
}

// ------------------------------------------------------------------------------------------------ matching
// a candidate: the ground truth g (-1: none) with its intersection, union and ignore flag
struct Cand {
    i64 in, un;
    int g, ign;
};

// is `c` better than `best` in the header's order (non-ignored first, then larger IoU, then larger g)?  c.g >= 0.
__device__ __forceinline__ bool better(const Cand& c, const Cand& best)
{
    if (best.g < 0) return true;
    if (c.ign != best.ign) return c.ign < best.ign;
    const i64 l = c.in * best.un, r = best.in * c.un;
    return l > r || (l == r && c.g > best.g);
}

// grid (Q, T), 64 threads
__global__ __launch_bounds__(64) void match_kernel(const int* __restrict__ det_off, const int* __restrict__ gt_off, const int* __restrict__ pair_off,
                                                   const i64* __restrict__ inter, int total_pair, const i64* __restrict__ area_det, int total_det,
                                                   const i64* __restrict__ area_gt, const unsigned char* __restrict__ gt_ignore, int total_gt,
                                                   const int* __restrict__ thr_num, i64 den, int* __restrict__ dt_match,
                                                   unsigned char* __restrict__ dt_ignore, int* __restrict__ status)
{
    const int q = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const int d0 = det_off[q], d1 = det_off[q + 1], g0 = gt_off[q], g1 = gt_off[q + 1], po = pair_off[q];
    const i64 D = (i64)d1 - d0, G = (i64)g1 - g0;
    if (!(0 <= d0 && d0 <= d1 && d1 <= total_det && 0 <= g0 && g0 <= g1 && g1 <= total_gt && po >= 0 && (i64)po + D * G <= (i64)total_pair)) {
        if (lane == 0 && t == 0) status[q] = GPC_GROUP_RANGE;         // D * G < 2^62: no wrap
        return;
    }
    int flag = 0;
    if (G > GPC_MAX_GROUP_GT) flag = GPC_GROUP_SIZE;
    else {
        int bad = 0;
        for (int g = 1 + lane; g < G; g += 64) bad |= gt_ignore[g0 + g - 1] != 0 && gt_ignore[g0 + g] == 0;
        if (__any(bad)) flag = GPC_GROUP_ORDER;
    }
    if (lane == 0 && t == 0) status[q] = flag;
    int* match_row = dt_match + (size_t)t * (size_t)total_det + d0;
    unsigned char* ignore_row = dt_ignore + (size_t)t * (size_t)total_det + d0;
    if (flag) {                                                       // uniform over the wave
        for (int d = lane; d < D; d += 64) match_row[d] = -1, ignore_row[d] = 0;
        return;
    }
    const i64 num = thr_num[t];
    u64 matched = 0;                                                  // bit k: ground truth lane + 64 k
    for (int d = 0; d < D; ++d) {
        const i64 ad = area_det[d0 + d];
        const i64* row = inter + (size_t)po + (size_t)d * (size_t)G;
        Cand best = {0, 1, -1, 0};
        for (int k = 0, g = lane; g < G; ++k, g += 64) {              // g ascending within the lane
            if ((matched >> k) & 1) continue;
            Cand c;
            c.in = row[g], c.un = ad + area_gt[g0 + g] - c.in, c.g = g, c.ign = gt_ignore[g0 + g] != 0;
            if (c.un <= 0 || c.in * den < num * c.un) continue;
            if (better(c, best)) best = c;
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
            Cand o;
            o.in = __shfl_xor(best.in, w, 64), o.un = __shfl_xor(best.un, w, 64), o.g = __shfl_xor(best.g, w, 64), o.ign = __shfl_xor(best.ign, w, 64);
            if (o.g >= 0 && better(o, best)) best = o;                // a total order on distinct g: every lane ends with the same one
        }
        if (lane == 0) match_row[d] = best.g, ignore_row[d] = (unsigned char)(best.g >= 0 ? best.ign : 0);
        if (best.g >= 0 && (best.g & 63) == lane) matched |= 1ull << (best.g >> 6);
    }
}

// ------------------------------------------------------------------------------------------------ suppression bits
// grid (words, ceil(P / 4))
__global__ __launch_bounds__(kThreads) void sup_bits_kernel(const i64* __restrict__ inter, const i64* __restrict__ area, int P, int words, i64 num,
                                                            i64 den, u64* __restrict__ sup)
{
    const int lane = threadIdx.x & 63, w = blockIdx.x;
    const int i = blockIdx.y * kWaves + ((int)threadIdx.x >> 6);
    if (i >= P) return;                                               // the whole wave
    const int j = w * 64 + lane;
    bool hit = false;
    if (j > i && j < P) {
        const i64 in = inter[(size_t)i * P + j];
        hit = in * den > num * (area[i] + area[j] - in);
    }
    const u64 word = __ballot(hit);
    if (lane == 0) sup[(size_t)i * words + w] = word;
}

}  // namespace

extern "C" {

int gpc_abi_version(void) { return 1; }

int gpc_fg_scan(const int* cum, const int* offsets, int total, int D, int HW, int* fg, long long* area, int* status, void* stream)
{
    GPF_REQUIRE(D >= 0 && D <= GPC_MAX_ITEMS && HW > 0 && total >= 0, "gpc_fg_scan: bad sizes (0 <= D <= 65535, 0 < HW < 2^31, total >= 0)");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(((cum && fg) || !total) && offsets && area && status, "gpc_fg_scan: null pointer (cum and fg may be null only when total is 0)");
    GPF_REQUIRE(((uintptr_t)area & 7) == 0, "gpc_fg_scan: area is not 8-byte aligned");
    hipLaunchKernelGGL(fg_scan_kernel, dim3(D), dim3(kThreads), 0, (hipStream_t)stream, cum, offsets, total, HW, fg, area, status);
    GPF_CHECK_LAUNCH("gpc_fg_scan");
    return GPF_OK;
}

int gpc_mask_inter(const int* cumA, const int* offA, const int* fgA, int totalA, int DA, const int* cumB, const int* offB, const int* fgB,
                   int totalB, int DB, int HW, const int* pair_a, const int* pair_b, int P, long long* inter, int* status, void* stream)
{
    GPF_REQUIRE(P >= 0 && P <= GPC_MAX_ITEMS, "gpc_mask_inter: P = %d pairs in one call (0 to 65535)", P);
    GPF_REQUIRE(DA >= 0 && DB >= 0 && totalA >= 0 && totalB >= 0 && HW > 0, "gpc_mask_inter: bad sizes (DA, DB, totalA, totalB >= 0, 0 < HW < 2^31)");
    if (P == 0) return GPF_OK;
    GPF_REQUIRE(((cumA && fgA) || !totalA) && ((cumB && fgB) || !totalB) && offA && offB && pair_a && pair_b && inter && status,
                "gpc_mask_inter: null pointer (cum and fg may be null only when their total is 0)");
    GPF_REQUIRE(((uintptr_t)inter & 7) == 0, "gpc_mask_inter: inter is not 8-byte aligned");
    hipLaunchKernelGGL(mask_inter_kernel, dim3((P + kWaves - 1) / kWaves), dim3(kThreads), 0, (hipStream_t)stream, cumA, offA, fgA, totalA, DA, cumB,
                       offB, fgB, totalB, DB, HW, pair_a, pair_b, P, inter, status);
    GPF_CHECK_LAUNCH("gpc_mask_inter");
    return GPF_OK;
}

int gpc_box_inter(const int* boxA, int DA, const int* boxB, int DB, const int* pair_a, const int* pair_b, int P, long long* inter,
                  long long* area_a, long long* area_b, int* status, void* stream)
{
    GPF_REQUIRE(P >= 0 && P <= GPC_MAX_ITEMS, "gpc_box_inter: P = %d pairs in one call (0 to 65535)", P);
    GPF_REQUIRE(DA >= 0 && DB >= 0, "gpc_box_inter: bad sizes (DA, DB >= 0)");
    if (P == 0) return GPF_OK;
    GPF_REQUIRE((boxA || !DA) && (boxB || !DB) && pair_a && pair_b && inter && area_a && area_b && status, "gpc_box_inter: null pointer (a set may be null only when it is empty)");
    GPF_REQUIRE((((uintptr_t)inter | (uintptr_t)area_a | (uintptr_t)area_b) & 7) == 0, "gpc_box_inter: inter, area_a or area_b is not 8-byte aligned");
    hipLaunchKernelGGL(box_inter_kernel, dim3((P + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, boxA, DA, boxB, DB, pair_a,
                       pair_b, P, inter, area_a, area_b, status);
    GPF_CHECK_LAUNCH("gpc_box_inter");
    return GPF_OK;
}

int gpc_match(const int* det_off, const int* gt_off, const int* pair_off, int Q, const long long* inter, int total_pair, const long long* area_det,
              int total_det, const long long* area_gt, const unsigned char* gt_ignore, int total_gt, const int* thr_num, int T, int thr_den,
              int* dt_match, unsigned char* dt_ignore, int* status, void* stream)
{
    GPF_REQUIRE(Q >= 0 && Q <= GPC_MAX_ITEMS, "gpc_match: Q = %d groups in one call (0 to 65535)", Q);
    GPF_REQUIRE(T >= 1 && T <= GPC_MAX_THRESHOLDS, "gpc_match: T = %d thresholds (1 to 16)", T);
    GPF_REQUIRE(thr_den >= 1 && thr_den <= GPC_MAX_DEN, "gpc_match: thr_den = %d (1 to 2^16)", thr_den);
    GPF_REQUIRE(total_pair >= 0 && total_det >= 0 && total_gt >= 0, "gpc_match: bad sizes (total_pair, total_det, total_gt >= 0)");
    if (Q == 0) return GPF_OK;
    GPF_REQUIRE(det_off && gt_off && pair_off && thr_num && status, "gpc_match: null pointer");
    GPF_REQUIRE((inter || !total_pair) && ((area_det && dt_match && dt_ignore) || !total_det) && ((area_gt && gt_ignore) || !total_gt),
                "gpc_match: null pointer (an array may be null only when its total is 0)");
    GPF_REQUIRE((((uintptr_t)inter | (uintptr_t)area_det | (uintptr_t)area_gt) & 7) == 0, "gpc_match: inter, area_det or area_gt is not 8-byte aligned");
    hipLaunchKernelGGL(match_kernel, dim3(Q, T), dim3(64), 0, (hipStream_t)stream, det_off, gt_off, pair_off, inter, total_pair, area_det, total_det,
                       area_gt, gt_ignore, total_gt, thr_num, (long long)thr_den, dt_match, dt_ignore, status);
    GPF_CHECK_LAUNCH("gpc_match");
    return GPF_OK;
}

int gpc_sup_bits(const long long* inter, const long long* area, int P, int num, int den, unsigned long long* sup, void* stream)
{
    GPF_REQUIRE(P >= 0 && P <= GPC_MAX_NMS, "gpc_sup_bits: P = %d masks (0 to 2048)", P);
    GPF_REQUIRE(den >= 1 && den <= GPC_MAX_DEN && num >= 0 && num <= den, "gpc_sup_bits: bad threshold %d / %d (0 <= num <= den, 1 <= den <= 2^16)", num, den);
    if (P == 0) return GPF_OK;
    GPF_REQUIRE(inter && area && sup, "gpc_sup_bits: null pointer");
    GPF_REQUIRE((((uintptr_t)inter | (uintptr_t)area | (uintptr_t)sup) & 7) == 0, "gpc_sup_bits: inter, area or sup is not 8-byte aligned");
    const int words = (P + 63) / 64;
    hipLaunchKernelGGL(sup_bits_kernel, dim3(words, (P + kWaves - 1) / kWaves), dim3(kThreads), 0, (hipStream_t)stream, inter, area, P, words,
                       (long long)num, (long long)den, sup);
    GPF_CHECK_LAUNCH("gpc_sup_bits");
    return GPF_OK;
}

}  // extern "C"
