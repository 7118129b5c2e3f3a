// libgigapose_appear.so (C-ABI: include/gigapose_appear.h): the appearance score of a mask proposal.  The patch tokens of a crop
// after the final LayerNorm, L2-normalised, quantised and split into three int8 limbs; the patches a crop's mask occupies; per
// (proposal, template) pair the 256 x 256 x C exact products on the int8 matrix cores, the masked maximum over the template's
// patches, the sum over the proposal's.
//   reference: none -- the reference holds no such stage; the header's definitions are the contract.
// token_kernel: grid (B * 256 / 64), 256 threads; lane l of wave j keeps chain S_j of token l (channels j, j + 4, ..), the four
// chains of a token meet in LDS as (S0 + S1) + (S2 + S3); the element-wise last pass gives wave j the 16-channel groups j, j + 4,
// .., a lane writes 16 bytes per limb plane.  Nothing is kept between the passes but three doubles: x is read four times.
// valid_kernel: grid (B), a thread per patch counts its 14 x 14 pixels.
// pair_kernel: grid (P), 256 threads: the pair's indices, its number of valid query patches, whether the template has one;
// writes status, n and sum = 0.  strip_kernel: grid (4, P), 256 threads = 4 waves; the workgroup owns 64 query patches (4 tiles of
// 16), wave w the template's patch tiles w, w + 4, w + 8, w + 12.  Per template tile: 4 query tiles x 5 weights x 4 = 80 int32
// accumulators; per 64 channels 12 + 48 operand registers (16 bytes a lane and limb, straight from global memory: a pair's limbs
// are 1.5 MB at C = 1024 and stay in L2, the strip's in L1) and 36 v_mfma_i32_16x16x64_i8.  The bank is operand A (rows j = 4 *
// (lane >> 4) + reg), the query operand B (columns i = lane & 15): a lane sees the j's of one i and keeps the running maximum of
// the header's 64-bit key; two shuffles join the four lane groups, LDS the four waves.  No LDS operand staging, no scratch.
// Only integers decide.  The one atomic is the integer add that joins a pair's four strip sums.  gigapose_testing/appear_ref.py
// restates the arithmetic; the two agree bit for bit.  The host-side plumbing is gp_front.h's, root gp_root.h's.  This library
// links no object of the other libraries and exports only gpp_* names.
#include <limits.h>
#include <math.h>

#include "gigapose_appear.h"   // the C ABI these definitions are compiled against
#define GP_FRONT_PREFIX gpp
#include "../gp_front.h"
#include "../gp_root.h"

namespace {

typedef unsigned long long u64;
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSide = 16;                            // patches along a side of the crop
constexpr int kCrop = kSide * GPP_CELL;              // 224
constexpr int kStrip = 64;                           // query patches of a strip_kernel workgroup
constexpr int kStrips = GPP_PATCHES / kStrip;
constexpr int kTile = 16;                            // the MFMA's M and N
constexpr int kStep = 64;                            // its K
constexpr int kQTiles = kStrip / kTile;              // query tiles of a wave
constexpr int kTTiles = GPP_PATCHES / kTile;         // template tiles of a pair
static_assert(kSide * kSide == GPP_PATCHES && kWaves == 4 && kStrips == 4 && kQTiles == 4 && kTTiles % kWaves == 0, "the shapes below");

// ------------------------------------------------------------------------------------------------ patch descriptors
// SUM of the header for the token of this lane: `s` is chain S_wave; returns (S0 + S1) + (S2 + S3) to all four waves.  Two
// barriers frame the exchange, so the array may be handed to the next call at once.
__device__ __forceinline__ double token_sum(double s, double (*part)[64])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    part[wave][lane] = s;
    __syncthreads();
    return (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// the balanced base-128 digits of q in [-2^20, 2^20]
__device__ __forceinline__ void limbs_of(int q, int& a0, int& a1, int& a2)
{
    a0 = ((q + 64) & 127) - 64;
    const int q1 = (q - a0) >> 7;                                     // exact: q - a0 is a multiple of 128
    a1 = ((q1 + 64) & 127) - 64;
    a2 = (q1 - a1) >> 7;
}

// grid (B * 4): 64 tokens a workgroup
__global__ __launch_bounds__(kThreads) void token_kernel(const float* __restrict__ x, long long crop_stride, long long token_stride,
                                                         long long channel_stride, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         double eps, int C, size_t plane, signed char* __restrict__ a, int* __restrict__ status)
{
    __shared__ double part[kWaves][64];
    __shared__ int flags[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t token = (size_t)blockIdx.x * 64 + lane;              // < B * 256 <= 2^28
    const size_t b = token / GPP_PATCHES, n = token % GPP_PATCHES;
    const float* row = x + b * (size_t)crop_stride + n * (size_t)token_stride;
    const size_t cs = (size_t)channel_stride;
    int bad = 0;
    double s = 0.0;
    for (int c = wave; c < C; c += 4) {
        const double v = (double)row[c * cs];
        bad |= !(fabs(v) < (double)INFINITY);
        s += v;
    }
    flags[wave][lane] = bad;                                          // read after token_sum's barriers
    const double mean = token_sum(s, part) / (double)C;
    bad = flags[0][lane] | flags[1][lane] | flags[2][lane] | flags[3][lane];
    s = 0.0;
    for (int c = wave; c < C; c += 4) {
        const double dev = (double)row[c * cs] - mean;
        s += dev * dev;
    }
    const double var = token_sum(s, part) / (double)C;
    const double r = 1.0 / root(var + eps);
    s = 0.0;
    for (int c = wave; c < C; c += 4) {
        const double y = (((double)row[c * cs] - mean) * r) * (double)gamma[c] + (double)beta[c];
        s += y * y;
    }
    const double n2 = token_sum(s, part);
    int flag = 0;
    if (bad || !(fabs(n2) < (double)INFINITY)) flag = GPP_NON_FINITE;
    else if (n2 == 0.0) flag = GPP_ZERO_NORM;
    const double norm = flag ? 1.0 : root(n2);
    signed char* out = a + token * (size_t)C;
    for (int c0 = wave * 16; c0 < C; c0 += 4 * 16) {                  // element-wise: any split over the waves gives the same bytes
        v4i w0, w1, w2;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned p0 = 0, p1 = 0, p2 = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + 4 * g + e;
                const double y = (((double)row[c * cs] - mean) * r) * (double)gamma[c] + (double)beta[c];
                const int q = flag ? 0 : (int)rint((y / norm) * 1048576.0);
                int a0, a1, a2;
                limbs_of(q, a0, a1, a2);
                p0 |= (unsigned)(a0 & 255) << (8 * e), p1 |= (unsigned)(a1 & 255) << (8 * e), p2 |= (unsigned)(a2 & 255) << (8 * e);
            }
            w0[g] = (int)p0, w1[g] = (int)p1, w2[g] = (int)p2;
        }
        *reinterpret_cast<v4i*>(out + c0) = w0;                      // a is 16-byte aligned, C and c0 multiples of 16
        *reinterpret_cast<v4i*>(out + plane + c0) = w1;
        *reinterpret_cast<v4i*>(out + 2 * plane + c0) = w2;
    }
    if (wave == 0) status[token] = flag;
}

// ------------------------------------------------------------------------------------------------ patch occupancy
// grid (B)
__global__ __launch_bounds__(kThreads) void valid_kernel(const float* __restrict__ mask, int num, int den, unsigned char* __restrict__ valid,
                                                         int* __restrict__ count, unsigned char* __restrict__ set)
{
    const size_t b = blockIdx.x;
    const int n = threadIdx.x, py = n / kSide, px = n % kSide;
    const float* cell = mask + b * (size_t)(kCrop * kCrop) + (size_t)(py * GPP_CELL) * kCrop + px * GPP_CELL;
    int k = 0;
    for (int y = 0; y < GPP_CELL; ++y)
#pragma unroll
        for (int xx = 0; xx < GPP_CELL; ++xx) k += cell[y * kCrop + xx] > 0.5f;
    const int ok = k * den > num * (GPP_CELL * GPP_CELL);             // k <= 196, den <= 2^16: below 2^24
    valid[b * GPP_PATCHES + n] = (unsigned char)ok;
    if (set) set[b * GPP_PATCHES + n] = (unsigned char)k;
    const int total = __syncthreads_count(ok);
    if (n == 0) count[b] = total;
}

// ------------------------------------------------------------------------------------------------ appearance
// grid (P)
__global__ __launch_bounds__(kThreads) void pair_kernel(const unsigned char* __restrict__ q_valid, int Bq, const unsigned char* __restrict__ t_valid,
                                                        int R, const int* __restrict__ qi, const int* __restrict__ ti, long long* __restrict__ sum,
                                                        int* __restrict__ n, int* __restrict__ status)
{
    const int p = blockIdx.x, t = threadIdx.x;
    const int q = qi[p], r = ti[p];
    int flag = 0, nq = 0;
    if (!(q >= 0 && q < Bq && r >= 0 && r < R)) flag = GPP_BAD_INDEX;  // uniform over the workgroup
    else {
        nq = __syncthreads_count(q_valid[(size_t)q * GPP_PATCHES + t] != 0);
        const int nt = __syncthreads_count(t_valid[(size_t)r * GPP_PATCHES + t] != 0);
        flag = (nq ? 0 : GPP_NO_QUERY_PATCH) | (nt ? 0 : GPP_NO_TEMPLATE_PATCH);
    }
    if (t == 0) sum[p] = 0, n[p] = flag ? 0 : nq, status[p] = flag;
}

__device__ __forceinline__ v4i load16(const signed char* p) { return *reinterpret_cast<const v4i*>(p); }

// grid (4, P): x the strip of 64 query patches
__global__ __launch_bounds__(kThreads, 2) void strip_kernel(const signed char* __restrict__ qa, const unsigned char* __restrict__ q_valid, size_t q_plane,
                                                         const signed char* __restrict__ ta, const unsigned char* __restrict__ t_valid, size_t t_plane,
                                                         int C, const int* __restrict__ qi, const int* __restrict__ ti,
                                                         const int* __restrict__ status, long long* __restrict__ sum, long long* __restrict__ best,
                                                         int* __restrict__ arg)
{
    __shared__ u64 keys[kWaves][kStrip];
    const int strip = blockIdx.x, p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const size_t out = (size_t)p * GPP_PATCHES + strip * kStrip + tid;  // of the threads tid < 64
    if (status[p] != 0) {                                             // pair_kernel's verdict, uniform: nothing of the pair is read
        if (tid < kStrip) {
            if (best) best[out] = 0;
            if (arg) arg[out] = -1;
        }
        return;
    }
    const size_t q = (size_t)qi[p], r = (size_t)ti[p];                 // in range: the pair is not flagged
    // lane (col, grp) holds bytes [16 * grp, 16 * grp + 16) of the step's 64 channels of row `col` of a tile -- of BOTH operands
    const signed char* qrow = qa + (q * GPP_PATCHES + strip * kStrip + col) * (size_t)C + 16 * grp;
    const signed char* trow = ta + (r * GPP_PATCHES + col) * (size_t)C + 16 * grp;
    const unsigned char* tv = t_valid + r * GPP_PATCHES;
    u64 top[kQTiles] = {0, 0, 0, 0};
    for (int jt = wave; jt < kTTiles; jt += kWaves) {
        v4i acc[kQTiles][5];
#pragma unroll
        for (int it = 0; it < kQTiles; ++it)
#pragma unroll
            for (int w = 0; w < 5; ++w) acc[it][w] = v4i{0, 0, 0, 0};
        const signed char* tt = trow + (size_t)(jt * kTile) * C;
        for (int c0 = 0; c0 < C; c0 += kStep) {
            v4i ta_[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) ta_[v] = load16(tt + v * t_plane + c0);
#pragma unroll
            for (int it = 0; it < kQTiles; ++it) {
                v4i qa_[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) qa_[u] = load16(qrow + u * q_plane + (size_t)(it * kTile) * C + c0);
#pragma unroll
                for (int u = 0; u < 3; ++u)
#pragma unroll
                    for (int v = 0; v < 3; ++v) acc[it][u + v] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ta_[v], qa_[u], acc[it][u + v], 0, 0, 0);
            }
        }
        // D: column = lane & 15 -> query patch, row = 4 * grp + reg -> template patch
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int j = jt * kTile + 4 * grp + reg;
            const bool live = tv[j] != 0;
#pragma unroll
            for (int it = 0; it < kQTiles; ++it) {
                const long long dot = (long long)acc[it][0][reg] + ((long long)acc[it][1][reg] << 7) + ((long long)acc[it][2][reg] << 14) +
                                      ((long long)acc[it][3][reg] << 21) + ((long long)acc[it][4][reg] << 28);
                const u64 key = live ? ((u64)(dot + (1ll << 52)) << 8) | (u64)(255 - j) : 0ull;
                top[it] = key > top[it] ? key : top[it];
            }
        }
    }
#pragma unroll
    for (int it = 0; it < kQTiles; ++it) {
#pragma unroll
        for (int w = 16; w <= 32; w <<= 1) {
            const u64 other = __shfl_xor(top[it], w, 64);
            top[it] = other > top[it] ? other : top[it];
        }
        if (grp == 0) keys[wave][it * kTile + col] = top[it];
    }
    __syncthreads();
    if (tid < kStrip) {                                               // wave 0: thread i of the strip
        u64 key = keys[0][tid];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) key = keys[w][tid] > key ? keys[w][tid] : key;
        const bool live = q_valid[q * GPP_PATCHES + strip * kStrip + tid] != 0;     // the template has a valid patch: key != 0
        long long v = live ? (long long)(key >> 8) - (1ll << 52) : 0;
        if (best) best[out] = v;
        if (arg) arg[out] = live ? 255 - (int)(key & 255) : -1;
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
        if (tid == 0 && v != 0) atomicAdd(reinterpret_cast<u64*>(sum + p), (u64)v);   // two's complement: the signed sum
    }
}

}  // namespace

extern "C" {

int gpp_abi_version(void) { return 1; }

int gpp_patch_descriptors(const float* x, long long crop_stride, long long token_stride, long long channel_stride, const float* gamma,
                          const float* beta, double eps, int B, int C, signed char* a, int* status, void* stream)
{
    GPF_REQUIRE(B >= 0 && B <= GPP_MAX_ROWS, "gpp_patch_descriptors: B = %d crops in one call (0 to 2^20)", B);
    GPF_REQUIRE(C >= 64 && C <= GPP_MAX_C && C % 64 == 0, "gpp_patch_descriptors: C = %d channels (a multiple of 64, 64 to 2048)", C);
    GPF_REQUIRE(crop_stride > 0 && token_stride > 0 && channel_stride > 0 && crop_stride < (1ll << 40) && token_stride < (1ll << 40) &&
                    channel_stride < (1ll << 40),
                "gpp_patch_descriptors: bad strides %lld, %lld, %lld (in elements, 0 < stride < 2^40)", crop_stride, token_stride, channel_stride);
    GPF_REQUIRE(eps >= 0.0 && eps < (double)INFINITY, "gpp_patch_descriptors: eps must be finite and >= 0");
    if (B == 0) return GPF_OK;
    GPF_REQUIRE(x && gamma && beta && a && status, "gpp_patch_descriptors: null pointer");
    GPF_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)a & 15) == 0, "gpp_patch_descriptors: x is not 4-byte or a is not 16-byte aligned");
    hipLaunchKernelGGL(token_kernel, dim3(B * (GPP_PATCHES / 64)), dim3(kThreads), 0, (hipStream_t)stream, x, crop_stride, token_stride, channel_stride,
                       gamma, beta, eps, C, (size_t)B * GPP_PATCHES * C, a, status);
    GPF_CHECK_LAUNCH("gpp_patch_descriptors");
    return GPF_OK;
}

int gpp_patch_valid(const float* mask, int B, int num, int den, unsigned char* valid, int* count, unsigned char* set, void* stream)
{
    GPF_REQUIRE(B >= 0 && B <= GPP_MAX_ROWS, "gpp_patch_valid: B = %d crops in one call (0 to 2^20)", B);
    GPF_REQUIRE(den >= 1 && den <= 65536 && num >= 0 && num <= den, "gpp_patch_valid: bad threshold %d / %d (0 <= num <= den, 1 <= den <= 2^16)", num, den);
    if (B == 0) return GPF_OK;
    GPF_REQUIRE(mask && valid && count, "gpp_patch_valid: null pointer (set alone is optional)");
    GPF_REQUIRE(((uintptr_t)mask & 3) == 0, "gpp_patch_valid: mask is not 4-byte aligned");
    hipLaunchKernelGGL(valid_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, mask, num, den, valid, count, set);
    GPF_CHECK_LAUNCH("gpp_patch_valid");
    return GPF_OK;
}

int gpp_appearance(const signed char* qa, const unsigned char* q_valid, int Bq, const signed char* ta, const unsigned char* t_valid, int R,
                   int C, const int* qi, const int* ti, int P, long long* sum, int* n, int* status, long long* best, int* arg, void* stream)
{
    GPF_REQUIRE(P >= 0 && P <= GPP_MAX_PAIRS, "gpp_appearance: P = %d pairs in one call (0 to 65535)", P);
    GPF_REQUIRE(Bq >= 1 && Bq <= GPP_MAX_ROWS && R >= 1 && R <= GPP_MAX_ROWS, "gpp_appearance: bad sizes Bq = %d crops, R = %d bank rows (1 to 2^20)", Bq, R);
    GPF_REQUIRE(C >= 64 && C <= GPP_MAX_C && C % 64 == 0, "gpp_appearance: C = %d channels (a multiple of 64, 64 to 2048)", C);
    if (P == 0) return GPF_OK;
    GPF_REQUIRE(qa && q_valid && ta && t_valid && qi && ti && sum && n && status, "gpp_appearance: null pointer (best and arg alone are optional)");
    GPF_REQUIRE(((uintptr_t)qa & 15) == 0 && ((uintptr_t)ta & 15) == 0, "gpp_appearance: qa or ta is not 16-byte aligned");
    GPF_REQUIRE(((uintptr_t)sum & 7) == 0 && ((uintptr_t)best & 7) == 0, "gpp_appearance: sum or best is not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pair_kernel, dim3(P), dim3(kThreads), 0, s, q_valid, Bq, t_valid, R, qi, ti, sum, n, status);
    GPF_CHECK_LAUNCH("gpp_appearance");
    hipLaunchKernelGGL(strip_kernel, dim3(kStrips, P), dim3(kThreads), 0, s, qa, q_valid, (size_t)Bq * GPP_PATCHES * C, ta, t_valid,
                       (size_t)R * GPP_PATCHES * C, C, qi, ti, status, sum, best, arg);
    GPF_CHECK_LAUNCH("gpp_appearance");
    return GPF_OK;
}

}  // extern "C"
