// libgigapose_gtinfo.so (C-ABI: include/gigapose_gtinfo.h): what scene_gt_info.json and the mask / mask_visib images of a BOP
// dataset hold, for ground truths drawn by the render library: pixel counts, boxes and run-length masks.
//   reference: bop_toolkit's calc_gt_info.py / calc_gt_masks.py are what the reference's datasets were made with; nothing of
//   them is restated here, the header's definitions are the contract.
// classify_kernel: grid (64 x 64 canvas tile, instance), 256 threads = 4 waves; a wave reads 64 consecutive keys of a row (512
// bytes), a thread 16 rows.  The sensor's depth and the ray are read for object pixels inside the frame only.  The class bytes go
// through an LDS tile (rows padded to 68 bytes: the transposed reads of a wave fall into 64 different banks) and leave as 64
// consecutive bytes of a column.  A tile that does not touch the frame only counts.  The four counters (at most 16 per thread)
// and the eight box corners are reduced by wave shuffles, then LDS, then one atomic per value that is not neutral.
// count_kernel / write_kernel: grid (chunk of 4096 column-major pixels, instance).  The chunk's bits and the one before it are
// laid into LDS by coalesced byte loads; a thread owns 16 consecutive pixels and keeps their transition flags in a 16-bit word.
// count_kernel leaves per chunk the number of transitions and the position of the last one; write_kernel sums / maximises the
// earlier chunks' entries (at most 1 024), scans the flags over the block (gp_rle_scan.h: block_inclusive) and the last
// positions with a maximum, and writes cum and counts of its transitions; the last thread of the last chunk closes the list.
// Only integers are merged; no float atomics.  gigapose_testing/gtinfo_ref.py restates the arithmetic in numpy; the two agree bit
// for bit.  The host-side plumbing is gp_front.h's, list_range and block_inclusive are gp_rle_scan.h's, the sums gp_key_walk.h's.
// This library links no object of the other libraries and exports only gpg_* names.
#include <math.h>

#include "gigapose_gtinfo.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpg
#include "../gp_front.h"
#include "../gp_key_walk.h"

namespace {

constexpr int kTile = 64;                     // a canvas tile is kTile x kTile pixels
constexpr int kTilePad = 4;
constexpr int kRunPix = 16;                   // consecutive column-major pixels of a thread
constexpr int kRunChunk = kScanThreads * kRunPix;
static_assert(kThreads == 256 && kWaves == 4 && kScanThreads == kThreads && kTile * kTile == kThreads * 16, "the shapes below");
static_assert(GPG_INFO == 4 && GPG_BOX == 8 && GPG_BOX_EMPTY_MIN == (1 << 30) && GPG_BOX_EMPTY_MAX == -(1 << 30), "the rows of info and box");
static_assert(kMaxPixels / kRunChunk == 1024, "a list has at most 1 024 chunks");

// grid (ceil(N / 256)): the initial values of info, box and status
__global__ __launch_bounds__(kThreads) void init_kernel(int N, long long* __restrict__ info, int* __restrict__ box, int* __restrict__ status)
{
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
#pragma unroll
    for (int i = 0; i < GPG_INFO; ++i) info[GPG_INFO * (size_t)n + i] = 0;
#pragma unroll
    for (int i = 0; i < GPG_BOX; ++i) box[GPG_BOX * (size_t)n + i] = (i & 2) ? GPG_BOX_EMPTY_MAX : GPG_BOX_EMPTY_MIN;
    status[n] = 0;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v = min(v, __shfl_xor(v, w, 64));
    return v;
}

// grid (tiles_x * tiles_y, N).  cls zeroed, info / box / status initialised by the caller
__global__ __launch_bounds__(kThreads) void classify_kernel(const u64* __restrict__ vis, int Hc, int Wc, int ox, int oy,
                                                            const float* __restrict__ depth, int M, const int* __restrict__ frame,
                                                            const double* __restrict__ ray, int R, const int* __restrict__ ray_index,
                                                            double delta, int H, int W, int tiles_x, unsigned char* __restrict__ cls,
                                                            long long* __restrict__ info, int* __restrict__ box, int* __restrict__ status)
{
    __shared__ long long part[kWaves][GPG_INFO];
    __shared__ int corner[kWaves][GPG_BOX];
    __shared__ unsigned char tile[kTile][kTile + kTilePad];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the pair rules: uniform over the workgroup and over the instance's workgroups, like every branch on `touches` below
    int bad = 0, fr = 0;
    if (depth) {
        fr = frame[n];
        if (fr < 0 || fr >= M) bad |= GPG_BAD_FRAME;
    }
    const int ri = ray_index[n];
    if (ri < 0 || ri >= R) bad |= GPG_BAD_RAY;
    if (bad) {
        if (tid == 0 && blockIdx.x == 0) atomicOr(status + n, bad);
        return;
    }
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTile, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTile;   // < Wc, Hc <= 2^30
    const bool touches = tx0 < ox + W && tx0 + kTile > ox && ty0 < oy + H && ty0 + kTile > oy;
    const u64* keys = vis + (size_t)n * Hc * Wc;
    const float* dmap = depth ? depth + (size_t)fr * H * W : nullptr;
    const double* rmap = ray + (size_t)ri * H * W;

    int acc[GPG_INFO] = {0, 0, 0, 0};
    int lo[4] = {GPG_BOX_EMPTY_MIN, GPG_BOX_EMPTY_MIN, GPG_BOX_EMPTY_MIN, GPG_BOX_EMPTY_MIN};    // min x, min y of the object, of the visible pixels
    int hi[4] = {GPG_BOX_EMPTY_MAX, GPG_BOX_EMPTY_MAX, GPG_BOX_EMPTY_MAX, GPG_BOX_EMPTY_MAX};    // max x, max y likewise
    const int cx = tx0 + lane, x = cx - ox;
    for (int s = 0; s < kTile / kWaves; ++s) {
        const int row = s * kWaves + wave, cy = ty0 + row, y = cy - oy;
        unsigned char b = 0;
        if (cx < Wc && cy < Hc) {
            const u64 key = keys[(size_t)cy * Wc + cx];
            const float dm = __uint_as_float((unsigned)(key >> 32));
            if (key != kEmptyKey && dm > 0.0f && dm < INFINITY) {                                // an object pixel
                acc[GPG_PX_ALL] += 1;
                lo[0] = min(lo[0], x), lo[1] = min(lo[1], y), hi[0] = max(hi[0], x), hi[1] = max(hi[1], y);
                if (x >= 0 && x < W && y >= 0 && y < H) {
                    const size_t at = (size_t)y * W + x;
                    float dt = 0.0f;
                    if (dmap) {
                        const float d = dmap[at];
                        dt = (d > 0.0f && d < INFINITY) ? d : 0.0f;
                    }
                    const double r = rmap[at];
                    const double Dm = (double)dm * r, Dt = (double)dt * r;
                    const bool visible = (dt > 0.0f && (Dm - Dt) <= delta) || dt == 0.0f;
                    acc[GPG_PX_FRAME] += 1;
                    acc[GPG_PX_VALID] += dt > 0.0f;
                    b = GPG_CLS_OBJECT;
                    if (visible) {
                        acc[GPG_PX_VISIB] += 1;
                        lo[2] = min(lo[2], x), lo[3] = min(lo[3], y), hi[2] = max(hi[2], x), hi[3] = max(hi[3], y);
                        b |= GPG_CLS_VISIBLE;
                    }
                }
            }
        }
        if (touches) tile[row][lane] = b;
    }
    wave_totals(acc, part);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lo[i] = wave_min(lo[i]);
        hi[i] = -wave_min(-hi[i]);
    }
    if (lane == 0) {
        // the order of a row of box: min x, min y, max x, max y of the object, then of the visible pixels
        corner[wave][0] = lo[0], corner[wave][1] = lo[1], corner[wave][2] = hi[0], corner[wave][3] = hi[1];
        corner[wave][4] = lo[2], corner[wave][5] = lo[3], corner[wave][6] = hi[2], corner[wave][7] = hi[3];
    }
    __syncthreads();
    if (tid < GPG_INFO) {
        const long long v = workgroup_total(part, tid);
        if (v) add_to_row(info, GPG_INFO, n, tid, v);
    } else if (tid >= 64 && tid < 64 + GPG_BOX) {
        const int i = tid - 64;
        int* out = box + GPG_BOX * (size_t)n + i;
        if (i & 2) {
            int v = GPG_BOX_EMPTY_MAX;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) v = max(v, corner[w][i]);
            if (v != GPG_BOX_EMPTY_MAX) atomicMax(out, v);
        } else {
            int v = GPG_BOX_EMPTY_MIN;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) v = min(v, corner[w][i]);
            if (v != GPG_BOX_EMPTY_MIN) atomicMin(out, v);
        }
    }
    if (!touches) return;
    // the tile transposed: a wave stores 64 consecutive pixels of a column
    unsigned char* out = cls + (size_t)n * W * H;
    const int fy = ty0 + lane - oy;
    for (int s = 0; s < kTile / kWaves; ++s) {
        const int col = s * kWaves + wave, fx = tx0 + col - ox;
        if (fx >= 0 && fx < W && fy >= 0 && fy < H) out[(size_t)fx * H + fy] = tile[lane][col];
    }
}

// The chosen bit of the chunk's pixels and of the pixel before the chunk, laid into LDS (bit[i] = v(base - 1 + i), 0 outside
// [0, HW)); -> the transition flags of this thread's kRunPix consecutive pixels from `first` on, flag k for pixel first + k.
// Holds a barrier: every thread of the block calls it.
__device__ __forceinline__ unsigned transition_flags(const unsigned char* __restrict__ src, int HW, int base, int which, unsigned char* bit,
                                                     int& first)
{
    for (int i = threadIdx.x; i <= kRunChunk; i += kScanThreads) {
        const int p = base - 1 + i;                                     // < 2^22 + 4096
        bit[i] = (p >= 0 && p < HW) ? (unsigned char)((src[p] >> which) & 1) : (unsigned char)0;
    }
    __syncthreads();
    const int mine = (int)threadIdx.x * kRunPix;
    first = base + mine;
    unsigned f = 0;
#pragma unroll
    for (int k = 0; k < kRunPix; ++k)
        if (first + k < HW && bit[mine + k + 1] != bit[mine + k]) f |= 1u << k;
    return f;
}

// the position of the last transition among the flags, 0 without any (the identity of the maximum: positions are >= 0)
__device__ __forceinline__ int last_position(unsigned f, int first) { return f ? first + (31 - __clz((int)f)) : 0; }

// grid (chunks, N).  runs zeroed by the caller; work[n * chunks + c] = (transitions of chunk c, position of its last one)
__global__ __launch_bounds__(kScanThreads) void count_kernel(const unsigned char* __restrict__ cls, int HW, int which, int chunks,
                                                             int* __restrict__ runs, int2* __restrict__ work)
{
    __shared__ unsigned char bit[kRunChunk + 1];
    __shared__ int slot[2][kScanWaves];
    const int n = blockIdx.y, c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int first;
    const unsigned f = transition_flags(cls + (size_t)n * HW, HW, c * kRunChunk, which, bit, first);
    const int count = wave_sum((int)__popc(f));
    const int last = -wave_min(-last_position(f, first));
    if (lane == 0) slot[0][wave] = count, slot[1][wave] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0, at = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) total += slot[0][w], at = max(at, slot[1][w]);
        work[(size_t)n * chunks + c] = make_int2(total, at);
        atomicAdd(runs + n, total + (c == 0));                          // + 1: the list's last entry
    }
}

// grid (chunks, N)
__global__ __launch_bounds__(kScanThreads) void write_kernel(const unsigned char* __restrict__ cls, int HW, int which, int chunks,
                                                             const int2* __restrict__ work, const int* __restrict__ offsets, int total,
                                                             int* __restrict__ counts, int* __restrict__ cum, int* __restrict__ err)
{
    __shared__ unsigned char bit[kRunChunk + 1];
    __shared__ int red[3][kScanWaves];
    __shared__ int slot[kScanWaves], top[kScanWaves];
    const int n = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // over the instance's chunks: all transitions (the list's length - 1), those of the earlier chunks (this chunk's base
    // rank) and the position of the last transition before this chunk
    int all = 0, before = 0, prev = 0;
    for (int i = tid; i < chunks; i += kScanThreads) {
        const int2 w = work[(size_t)n * chunks + i];
        all += w.x;
        if (i < c) before += w.x, prev = max(prev, w.y);
    }
    all = wave_sum(all), before = wave_sum(before), prev = -wave_min(-prev);
    if (lane == 0) red[0][wave] = all, red[1][wave] = before, red[2][wave] = prev;
    __syncthreads();
    all = before = prev = 0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) all += red[0][w], before += red[1][w], prev = max(prev, red[2][w]);
    int lo, hi;
    if (!list_range(offsets, n, total, lo, hi) || hi - lo != all + 1) {   // uniform over the instance's workgroups; 0 <= lo < hi <= total where compared
        if (c == 0 && tid == 0) atomicExch(err, n + 1);
        return;
    }
    int first;
    const unsigned f = transition_flags(cls + (size_t)n * HW, HW, c * kRunChunk, which, bit, first);
    const int mine = (int)__popc(f);
    int carry = before;
    int rank = block_inclusive(mine, carry, slot, lane, wave) - mine;   // of this thread's first transition among the instance's
    // the position of the last transition before this thread's pixels: a maximum scan, `prev` in front
    int upto = last_position(f, first);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(upto, off);
        if (lane >= off) upto = max(upto, o);
    }
    if (lane == 63) top[wave] = upto;
    int last = __shfl_up(upto, 1);
    if (lane == 0) last = 0;
    __syncthreads();
    last = max(last, prev);
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w)
        if (w < wave) last = max(last, top[w]);
    const int room = hi - lo - 1;                                       // the transitions' part of the slice
#pragma unroll
    for (int k = 0; k < kRunPix; ++k) {
        if (!((f >> k) & 1)) continue;
        const int p = first + k;
        if (rank < room) {                                              // always, by the count: the rank is never trusted
            cum[lo + rank] = p;
            counts[lo + rank] = p - last;
        }
        last = p;
        ++rank;
    }
    if (c == chunks - 1 && tid == kScanThreads - 1) {                   // behind every transition of the instance
        cum[hi - 1] = HW;
        counts[hi - 1] = HW - last;
    }
}

inline int run_chunks(int H, int W) { return (int)(((long long)H * W + kRunChunk - 1) / kRunChunk); }

inline bool run_sizes_ok(int N, int H, int W) { return N >= 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W <= kMaxPixels; }

}  // namespace

extern "C" {

int gpg_abi_version(void) { return 1; }

int gpg_pixels_per_workgroup(void) { return kRunChunk; }

size_t gpg_runs_workspace_bytes(int N, int H, int W)
{
    if (!run_sizes_ok(N, H, W)) return 0;
    return (size_t)N * (size_t)run_chunks(H, W) * sizeof(int2);
}

int gpg_classify(const unsigned long long* vis, int Hc, int Wc, int ox, int oy, const float* depth, int M, const int* frame,
                 const double* ray, int R, const int* ray_index, double delta, int N, int H, int W, unsigned char* cls,
                 long long* info, int* box, int* status, void* stream)
{
    GPF_REQUIRE(N >= 0 && N <= 65535, "gpg_classify: N = %d instances in one call (0 to 65535)", N);
    GPF_REQUIRE(H > 0 && W > 0 && (long long)H * W <= kMaxPixels, "gpg_classify: bad frame %d x %d (H, W > 0, H*W <= 2^22)", H, W);
    GPF_REQUIRE(Hc > 0 && Wc > 0 && Hc <= (1 << 30) && Wc <= (1 << 30) && (long long)Hc * Wc < (1ll << 31),
                "gpg_classify: bad canvas %d x %d (Hc, Wc > 0, Hc, Wc <= 2^30, Hc*Wc < 2^31)", Hc, Wc);
    GPF_REQUIRE(ox >= 0 && oy >= 0 && (long long)ox + W <= Wc && (long long)oy + H <= Hc,
                "gpg_classify: the frame leaves the canvas (0 <= ox, ox + W <= Wc, 0 <= oy, oy + H <= Hc; ox = %d, oy = %d)", ox, oy);
    GPF_REQUIRE((!depth || M >= 1) && R >= 1, "gpg_classify: bad sizes (with depth M >= 1; R >= 1)");
    GPF_REQUIRE(delta == delta, "gpg_classify: delta is NaN");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(vis && ray && ray_index && cls && info && box && status && (!depth || frame),
                "gpg_classify: null pointer (frame is required with depth)");
    GPF_REQUIRE(((uintptr_t)vis & 7) == 0 && ((uintptr_t)info & 7) == 0, "gpg_classify: vis or info is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    GPF_CHECK_HIP("gpg_classify", hipMemsetAsync(cls, 0, (size_t)N * H * W, s));
    hipLaunchKernelGGL(init_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, s, N, info, box, status);
    GPF_CHECK_LAUNCH("gpg_classify");
    const int tiles_x = (Wc + kTile - 1) / kTile, tiles_y = (Hc + kTile - 1) / kTile;       // their product < 2^19 + 2^25
    hipLaunchKernelGGL(classify_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, N), dim3(kThreads), 0, s, vis, Hc, Wc, ox, oy, depth, M,
                       frame, ray, R, ray_index, delta, H, W, tiles_x, cls, info, box, status);
    GPF_CHECK_LAUNCH("gpg_classify");
    return GPF_OK;
}

int gpg_count_runs(const unsigned char* cls, int N, int H, int W, int which, int* runs, void* workspace, void* stream)
{
    GPF_REQUIRE(run_sizes_ok(N, H, W), "gpg_count_runs: bad sizes (0 <= N <= 65535, H, W > 0, H*W <= 2^22)");
    GPF_REQUIRE(which == 0 || which == 1, "gpg_count_runs: which must be 0 (the object bit) or 1 (the visible bit)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(cls && runs && workspace, "gpg_count_runs: null pointer");
    GPF_REQUIRE(((uintptr_t)workspace & 7) == 0, "gpg_count_runs: workspace is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int chunks = run_chunks(H, W);
    GPF_CHECK_HIP("gpg_count_runs", hipMemsetAsync(runs, 0, (size_t)N * sizeof(int), s));
    hipLaunchKernelGGL(count_kernel, dim3(chunks, N), dim3(kScanThreads), 0, s, cls, H * W, which, chunks, runs, reinterpret_cast<int2*>(workspace));
    GPF_CHECK_LAUNCH("gpg_count_runs");
    return GPF_OK;
}

int gpg_write_runs(const unsigned char* cls, int N, int H, int W, int which, const void* workspace, const int* offsets, int total,
                   int* counts, int* cum, int* err, void* stream)
{
    GPF_REQUIRE(run_sizes_ok(N, H, W) && total >= 0, "gpg_write_runs: bad sizes (0 <= N <= 65535, H, W > 0, H*W <= 2^22, total >= 0)");
    GPF_REQUIRE(which == 0 || which == 1, "gpg_write_runs: which must be 0 (the object bit) or 1 (the visible bit)");
    if (N == 0) return GPF_OK;
    GPF_REQUIRE(cls && workspace && offsets && counts && cum && err, "gpg_write_runs: null pointer");
    GPF_REQUIRE(((uintptr_t)workspace & 7) == 0, "gpg_write_runs: workspace is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int chunks = run_chunks(H, W);
    GPF_CHECK_HIP("gpg_write_runs", hipMemsetAsync(err, 0, sizeof(int), s));
    hipLaunchKernelGGL(write_kernel, dim3(chunks, N), dim3(kScanThreads), 0, s, cls, H * W, which, chunks, reinterpret_cast<const int2*>(workspace),
                       offsets, total, counts, cum, err);
    GPF_CHECK_LAUNCH("gpg_write_runs");
    return GPF_OK;
}

}  // extern "C"
