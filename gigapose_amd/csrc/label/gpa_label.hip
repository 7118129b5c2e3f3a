// libgigapose_label.so (C-ABI: include/gigapose_label.h): mask proposals -> labelled detections.  The descriptor of a crop (the
// ViT's class token after the final LayerNorm, L2-normalised, quantised), its similarity with every template of every object,
// the object's top-k score and the label; the tight boxes of run-length masks; a greedy box NMS.
//   reference: none -- the reference starts from CNOS's labelled detections; the header's definitions are the contract.
// descriptor_kernel: grid (crop), 256 threads; a thread keeps its <= 8 channels in registers as float64; three block sums in the
// header's order (sequential per thread, then a pairwise tree over the 256 partials in LDS); the two roots are gp_root.h's.
// dots_kernel: grid (64 bank rows, 64 proposals), 256 threads; q and the bank go through LDS 32 channels at a time, transposed
// (channel-major, rows padded to 68 words: a thread reads its four rows as one 16-byte word); a thread holds 4 x 4 int64 sums.
// select_kernel: grid (proposal), a wave per object in turn; kk passes over the object's dots, each taking the largest (value,
// then smallest t) below the one taken before, so equal dots are taken once each and nothing is stored; the waves' best objects
// meet in LDS.  run_boxes_kernel: grid (detection), the runs of ones strided over the threads, closed form per run.
// nms_matrix_kernel: grid (column word, row block), 64 threads, a thread one row and 64 columns from LDS.  nms_keep_kernel: one
// workgroup; per block of 64 rows every thread resolves the block's diagonal words (uniformly, from LDS), then thread w folds the
// kept rows into the removed word w it owns.
// Only integers decide; no float atomics, no atomics at all.  gigapose_testing/label_ref.py restates the arithmetic; the two
// agree bit for bit.  The host-side plumbing is gp_front.h's, list_range gp_rle_scan.h's, root gp_root.h's.  This library links
// no object of the other libraries and exports only gpa_* names.
#include <limits.h>
#include <math.h>

#include "gigapose_label.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpa
#include "../gp_front.h"
#include "../gp_rle_scan.h"
#include "../gp_root.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = GPA_MAX_C / kThreads;     // channels of a thread in descriptor_kernel
constexpr int kTile = 64;                            // dots_kernel: proposals x bank rows of a workgroup
constexpr int kTileK = 32;                           // channels per LDS slab
constexpr int kTilePad = 4;
constexpr int kMaxWords = GPA_MAX_NMS / 64;
static_assert(kPerThread == 8 && kMaxWords <= kThreads && kTile * kTile == kThreads * 16, "the shapes below");

// ------------------------------------------------------------------------------------------------ descriptors
// SUM of the header: `v` is this thread's partial; returns partial[0] to every thread.  Two barriers frame the tree, so the
// array may be handed to the next call at once.
__device__ __forceinline__ double block_sum(double v, double* part)
{
    const int t = threadIdx.x;
    __syncthreads();
    part[t] = v;
    __syncthreads();
    for (int off = kThreads / 2; off >= 1; off >>= 1) {
        if (t < off) part[t] += part[t + off];
        __syncthreads();
    }
    return part[0];
}

// grid (B)
__global__ __launch_bounds__(kThreads) void descriptor_kernel(const float* __restrict__ x, long long crop_stride, long long channel_stride,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, double eps, int C,
                                                              int* __restrict__ q, int* __restrict__ status)
{
    __shared__ double part[kThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* row = x + (size_t)b * (size_t)crop_stride;
    double v[kPerThread];
    int bad = 0;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int c = t + i * kThreads;
        v[i] = 0.0;
        if (c < C) {
            v[i] = (double)row[(size_t)c * (size_t)channel_stride];
            bad |= !(fabs(v[i]) < (double)INFINITY);
            s += v[i];
        }
    }
    bad = __syncthreads_or(bad);
    const double mean = block_sum(s, part) / (double)C;
    s = 0.0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
        if (t + i * kThreads < C) {
            v[i] = v[i] - mean;
            s += v[i] * v[i];
        }
    const double var = block_sum(s, part) / (double)C;
    const double r = 1.0 / root(var + eps);
    s = 0.0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int c = t + i * kThreads;
        if (c < C) {
            v[i] = (v[i] * r) * (double)gamma[c] + (double)beta[c];
            s += v[i] * v[i];
        }
    }
    const double n2 = block_sum(s, part);
    int flag = 0;
    if (bad || !(fabs(n2) < (double)INFINITY)) flag = GPA_NON_FINITE;
    else if (n2 == 0.0) flag = GPA_ZERO_NORM;
    const double norm = flag ? 1.0 : root(n2);
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int c = t + i * kThreads;
        if (c < C) q[(size_t)b * C + c] = flag ? 0 : (int)rint((v[i] / norm) * 1048576.0);
    }
    if (t == 0) status[b] = flag;
}

// ------------------------------------------------------------------------------------------------ scores
// rows [r0, r0 + 64) x channels [c0, c0 + 32) of a (R, C) int32 matrix -> slab[channel][row], 0 outside the matrix
__device__ __forceinline__ void load_slab(const int* __restrict__ m, int R, int C, int r0, int c0, int (*slab)[kTile + kTilePad])
{
#pragma unroll
    for (int s = 0; s < kTile * kTileK / kThreads; ++s) {
        const int e = (int)threadIdx.x + s * kThreads, r = e / kTileK, k = e % kTileK;
        const int row = r0 + r, c = c0 + k;                           // row < 2^20 + 64 or < P + 64; c < 2048 + 32
        slab[k][r] = (row < R && c < C) ? m[(size_t)row * C + c] : 0;
    }
}

// grid (ceil(N / 64), ceil(P / 64)); N = O * T bank rows
__global__ __launch_bounds__(kThreads) void dots_kernel(const int* __restrict__ q, const int* __restrict__ bank, int P, int N, int C,
                                                        long long* __restrict__ dot)
{
    __shared__ __attribute__((aligned(16))) int qs[kTileK][kTile + kTilePad];
    __shared__ __attribute__((aligned(16))) int bs[kTileK][kTile + kTilePad];
    const int n0 = blockIdx.x * kTile, p0 = blockIdx.y * kTile;
    const int ty = (int)threadIdx.x / 16 * 4, tx = (int)threadIdx.x % 16 * 4;
    long long acc[4][4] = {};
    for (int c0 = 0; c0 < C; c0 += kTileK) {
        __syncthreads();                                              // the slabs of the step before have been read
        load_slab(q, P, C, p0, c0, qs);
        load_slab(bank, N, C, n0, c0, bs);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kTileK; ++k) {
            const int4 a = *reinterpret_cast<const int4*>(&qs[k][ty]);
            const int4 b = *reinterpret_cast<const int4*>(&bs[k][tx]);
            const int av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += (long long)av[i] * (long long)bv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + i;
        if (p >= P) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx + j;
            if (n < N) dot[(size_t)p * N + n] = acc[i][j];
        }
    }
}

// the larger of two (value, index) pairs in the order (value, then SMALLER index), over the wave
__device__ __forceinline__ void wave_first_max(long long& v, int& at)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const long long ov = __shfl_xor(v, w, 64);
        const int oat = __shfl_xor(at, w, 64);
        if (ov > v || (ov == v && oat < at)) v = ov, at = oat;
    }
}

// grid (P)
__global__ __launch_bounds__(kThreads) void select_kernel(const long long* __restrict__ dot, int O, int T, int kk, long long* __restrict__ obj,
                                                          int* __restrict__ label, long long* __restrict__ score, int* __restrict__ best_template)
{
    __shared__ long long wsum[kWaves];
    __shared__ int wobj[kWaves], wtop[kWaves];
    const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long best_sum = LLONG_MIN;
    int best_o = INT_MAX, best_top = 0;
    for (int o = wave; o < O; o += kWaves) {                          // ascending: a strict comparison keeps the first
        const long long* row = dot + ((size_t)p * O + o) * T;
        long long sum = 0, prev_v = LLONG_MAX;
        int prev_t = -1, top = 0;
        for (int pass = 0; pass < kk; ++pass) {                       // kk <= T: every pass finds an element
            long long v = LLONG_MIN;
            int at = INT_MAX;
            for (int t = lane; t < T; t += 64) {
                const long long d = row[t];
                const bool open = d < prev_v || (d == prev_v && t > prev_t);
                if (open && (d > v || (d == v && t < at))) v = d, at = t;
            }
            wave_first_max(v, at);
            sum += v;
            if (pass == 0) top = at;
            prev_v = v, prev_t = at;
        }
        if (obj && lane == 0) obj[(size_t)p * O + o] = sum;
        if (sum > best_sum || best_o == INT_MAX) best_sum = sum, best_o = o, best_top = top;
    }
    if (lane == 0) wsum[wave] = best_sum, wobj[wave] = best_o, wtop[wave] = best_top;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (wobj[w] != INT_MAX && (wsum[w] > best_sum || (wsum[w] == best_sum && wobj[w] < best_o)))
                best_sum = wsum[w], best_o = wobj[w], best_top = wtop[w];
        label[p] = best_o, score[p] = best_sum, best_template[p] = best_top;      // O >= 1: wave 0 has an object
    }
}

// ------------------------------------------------------------------------------------------------ boxes of run-length masks
__device__ __forceinline__ int wave_min_int(int v)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v = min(v, __shfl_xor(v, w, 64));
    return v;
}

// grid (D)
__global__ __launch_bounds__(kThreads) void run_boxes_kernel(const int* __restrict__ cum, const int* __restrict__ offsets, int total, int H, int W,
                                                             int* __restrict__ box, long long* __restrict__ area, int* __restrict__ status)
{
    __shared__ int corner[kWaves][4];
    __shared__ long long count[kWaves];
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;                                             // < 2^31
    int lo, hi;
    if (!list_range(offsets, d, total, lo, hi) || cum[hi - 1] != HW) {  // uniform over the workgroup
        if (tid < 4) box[4 * (size_t)d + tid] = 0;
        if (tid == 0) area[d] = 0, status[d] = GPA_BAD_MASK;
        return;
    }
    int x0 = INT_MAX, y0 = INT_MAX, x1 = 0, y1 = 0;                   // the maxima are exclusive ends, >= 1 once a run is seen
    long long n = 0;
    for (long long i = (long long)lo + 1 + 2 * tid; i < hi; i += 2 * kThreads) {   // lo < i < hi <= total
        const int a = cum[i - 1], b = cum[i];
        if (!(0 <= a && a < b && b <= HW)) continue;
        const int xa = a / H, ya = a % H, xb = (b - 1) / H, yb = (b - 1) % H;
        n += b - a;
        x0 = min(x0, xa), x1 = max(x1, xb + 1);
        if (xa == xb) y0 = min(y0, ya), y1 = max(y1, yb + 1);
        else y0 = 0, y1 = H;
    }
    x0 = wave_min_int(x0), y0 = wave_min_int(y0), x1 = -wave_min_int(-x1), y1 = -wave_min_int(-y1);
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) n += __shfl_xor(n, w, 64);
    if (lane == 0) corner[wave][0] = x0, corner[wave][1] = y0, corner[wave][2] = x1, corner[wave][3] = y1, count[wave] = n;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            x0 = min(x0, corner[w][0]), y0 = min(y0, corner[w][1]), x1 = max(x1, corner[w][2]), y1 = max(y1, corner[w][3]), n += count[w];
        const bool empty = n == 0;
        int* out = box + 4 * (size_t)d;
        out[0] = empty ? 0 : x0, out[1] = empty ? 0 : y0, out[2] = empty ? 0 : x1, out[3] = empty ? 0 : y1;
        area[d] = n;
        status[d] = empty ? GPA_EMPTY_MASK : 0;
    }
}

// ------------------------------------------------------------------------------------------------ box NMS
__device__ __forceinline__ int clamp_coord(int v) { return min(max(v, -GPA_MAX_COORD), GPA_MAX_COORD); }

__device__ __forceinline__ long long box_area(int x0, int y0, int x1, int y1)
{
    return (long long)max(0, x1 - x0) * (long long)max(0, y1 - y0);   // each factor <= 2^22
}

// grid (words, words): x the column word, y the block of 64 rows; 64 threads
__global__ __launch_bounds__(64) void nms_matrix_kernel(const int* __restrict__ box, const int* __restrict__ label, int P, int words, long long num,
                                                        long long den, int per_label, u64* __restrict__ sup)
{
    __shared__ int cb[64][4];
    __shared__ int cl[64];
    const int bj = blockIdx.x, bi = blockIdx.y, r = threadIdx.x;
    const int row = bi * 64 + r, col = bj * 64 + r;
    if (bj < bi) {                                                    // below the diagonal: j < i everywhere
        if (row < P) sup[(size_t)row * words + bj] = 0;
        return;
    }
    if (col < P) {
#pragma unroll
        for (int i = 0; i < 4; ++i) cb[r][i] = clamp_coord(box[4 * (size_t)col + i]);
        cl[r] = per_label ? label[col] : 0;
    }
    __syncthreads();
    if (row >= P) return;
    int mine[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) mine[i] = clamp_coord(box[4 * (size_t)row + i]);
    const int my_label = per_label ? label[row] : 0;
    const long long my_area = box_area(mine[0], mine[1], mine[2], mine[3]);
    u64 word = 0;
    for (int c = 0; c < 64; ++c) {
        const int j = bj * 64 + c;
        if (j <= row || j >= P || cl[c] != my_label) continue;
        const long long inter = box_area(max(mine[0], cb[c][0]), max(mine[1], cb[c][1]), min(mine[2], cb[c][2]), min(mine[3], cb[c][3]));
        const long long uni = my_area + box_area(cb[c][0], cb[c][1], cb[c][2], cb[c][3]) - inter;
        if (inter * den > num * uni) word |= 1ull << c;
    }
    sup[(size_t)row * words + bj] = word;
}

// grid (1)
__global__ __launch_bounds__(kThreads) void nms_keep_kernel(const u64* __restrict__ sup, int P, int words, unsigned char* __restrict__ keep)
{
    __shared__ u64 removed[kMaxWords];
    __shared__ u64 diag[64];
    const int tid = threadIdx.x;
    if (tid < words) removed[tid] = 0;                                // words <= kMaxWords <= kThreads: thread w owns removed[w]
    for (int bi = 0; bi < words; ++bi) {
        __syncthreads();                                              // removed[bi] is final; diag of the block before has been read
        const int row0 = bi * 64;
        if (tid < 64) diag[tid] = row0 + tid < P ? sup[(size_t)(row0 + tid) * words + bi] : 0;
        __syncthreads();
        u64 cur = removed[bi];
        const int rows = min(64, P - row0);
        for (int r = 0; r < rows; ++r)                                // the same in every thread
            if (!((cur >> r) & 1)) cur |= diag[r];
        const u64 valid = rows == 64 ? ~0ull : (1ull << rows) - 1;
        const u64 kept = ~cur & valid;
        if (tid < rows) keep[row0 + tid] = (unsigned char)((kept >> tid) & 1);
        if (tid > bi && tid < words) {
            u64 acc = removed[tid];
            for (u64 m = kept; m; m &= m - 1) acc |= sup[(size_t)(row0 + (__ffsll((long long)m) - 1)) * words + tid];
            removed[tid] = acc;
        }
    }
}

}  // namespace

extern "C" {

int gpa_abi_version(void) { return 1; }

int gpa_descriptors(const float* x, long long crop_stride, long long channel_stride, const float* gamma, const float* beta, double eps,
                    int B, int C, int* q, int* status, void* stream)
{
    GPF_REQUIRE(B >= 0 && B <= (1 << 24), "gpa_descriptors: B = %d crops in one call (0 to 2^24)", B);
    GPF_REQUIRE(C >= 64 && C <= GPA_MAX_C && C % 64 == 0, "gpa_descriptors: C = %d channels (a multiple of 64, 64 to 2048)", C);
    GPF_REQUIRE(crop_stride > 0 && channel_stride > 0 && crop_stride < (1ll << 40) && channel_stride < (1ll << 40),
                "gpa_descriptors: bad strides %lld, %lld (in elements, 0 < stride < 2^40)", crop_stride, channel_stride);
    GPF_REQUIRE(eps >= 0.0 && eps < (double)INFINITY, "gpa_descriptors: eps must be finite and >= 0");
    if (B == 0) return GPF_OK;
    GPF_REQUIRE(x && gamma && beta && q && status, "gpa_descriptors: null pointer");
    GPF_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)q & 3) == 0, "gpa_descriptors: x or q is not 4-byte aligned");
    hipLaunchKernelGGL(descriptor_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, x, crop_stride, channel_stride, gamma, beta, eps, C, q,
                       status);
    GPF_CHECK_LAUNCH("gpa_descriptors");
    return GPF_OK;
}

int gpa_scores(const int* q, const int* bank, int P, int O, int T, int C, int k, long long* dot, long long* obj, int* label,
               long long* score, int* best_template, void* stream)
{
    GPF_REQUIRE(O >= 1 && T >= 1 && (long long)O * T <= GPA_MAX_BANK, "gpa_scores: bad bank %d objects x %d templates (O, T >= 1, O*T <= 2^20)", O, T);
    GPF_REQUIRE(P >= 0 && (long long)P * O * T < (1ll << 40), "gpa_scores: P = %d proposals (P >= 0, P*O*T < 2^40)", P);
    GPF_REQUIRE(C >= 1 && C <= GPA_MAX_C, "gpa_scores: C = %d channels (1 to 2048)", C);
    GPF_REQUIRE(k >= 1 && k <= GPA_MAX_K, "gpa_scores: k = %d (1 to 64)", k);
    if (P == 0) return GPF_OK;
    GPF_REQUIRE(q && bank && dot && label && score && best_template, "gpa_scores: null pointer (obj alone is optional)");
    GPF_REQUIRE(((uintptr_t)dot & 7) == 0 && ((uintptr_t)obj & 7) == 0 && ((uintptr_t)score & 7) == 0,
                "gpa_scores: dot, obj or score is not 8-byte aligned");
    GPF_REQUIRE(((uintptr_t)q & 3) == 0 && ((uintptr_t)bank & 3) == 0, "gpa_scores: q or bank is not 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int N = O * T;
    hipLaunchKernelGGL(dots_kernel, dim3((N + kTile - 1) / kTile, (P + kTile - 1) / kTile), dim3(kThreads), 0, s, q, bank, P, N, C, dot);
    GPF_CHECK_LAUNCH("gpa_scores");
    hipLaunchKernelGGL(select_kernel, dim3(P), dim3(kThreads), 0, s, dot, O, T, k < T ? k : T, obj, label, score, best_template);
    GPF_CHECK_LAUNCH("gpa_scores");
    return GPF_OK;
}

int gpa_run_boxes(const int* cum, const int* offsets, int total, int D, int H, int W, int* box, long long* area, int* status, void* stream)
{
    GPF_REQUIRE(frame_sizes_ok(D, H, W) && total >= 0, "gpa_run_boxes: bad sizes (0 <= D <= 65535, H, W > 0, H*W < 2^31, total >= 0)");
    if (D == 0) return GPF_OK;
    GPF_REQUIRE(cum && offsets && box && area && status, "gpa_run_boxes: null pointer");
    GPF_REQUIRE(((uintptr_t)area & 7) == 0, "gpa_run_boxes: area is not 8-byte aligned");
    hipLaunchKernelGGL(run_boxes_kernel, dim3(D), dim3(kThreads), 0, (hipStream_t)stream, cum, offsets, total, H, W, box, area, status);
    GPF_CHECK_LAUNCH("gpa_run_boxes");
    return GPF_OK;
}

int gpa_nms_matrix(const int* box, const int* label, int P, int num, int den, int per_label, unsigned long long* sup, void* stream)
{
    GPF_REQUIRE(P >= 0 && P <= GPA_MAX_NMS, "gpa_nms_matrix: P = %d boxes (0 to 8192)", P);
    GPF_REQUIRE(den >= 1 && den <= 65536 && num >= 0 && num <= den, "gpa_nms_matrix: bad threshold %d / %d (0 <= num <= den, 1 <= den <= 2^16)", num, den);
    if (P == 0) return GPF_OK;
    GPF_REQUIRE(box && sup && (label || !per_label), "gpa_nms_matrix: null pointer (label is required with per_label)");
    GPF_REQUIRE(((uintptr_t)sup & 7) == 0, "gpa_nms_matrix: sup is not 8-byte aligned");
    const int words = (P + 63) / 64;
    hipLaunchKernelGGL(nms_matrix_kernel, dim3(words, words), dim3(64), 0, (hipStream_t)stream, box, label, P, words, (long long)num, (long long)den,
                       per_label, sup);
    GPF_CHECK_LAUNCH("gpa_nms_matrix");
    return GPF_OK;
}

int gpa_nms_keep(const unsigned long long* sup, int P, unsigned char* keep, void* stream)
{
    GPF_REQUIRE(P >= 0 && P <= GPA_MAX_NMS, "gpa_nms_keep: P = %d boxes (0 to 8192)", P);
    if (P == 0) return GPF_OK;
    GPF_REQUIRE(sup && keep, "gpa_nms_keep: null pointer");
    GPF_REQUIRE(((uintptr_t)sup & 7) == 0, "gpa_nms_keep: sup is not 8-byte aligned");
    hipLaunchKernelGGL(nms_keep_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, sup, P, (P + 63) / 64, keep);
    GPF_CHECK_LAUNCH("gpa_nms_keep");
    return GPF_OK;
}

}  // extern "C"
