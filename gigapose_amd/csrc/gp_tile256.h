// The 256-tile protocol of the split-f16 plane kernels, defined ONCE: gemm_split256_kernel / gemm_planes256_kernel (gp_split256.hip) and
// conv_planes_kernel / conv_halo_kernel (gp_conv256.hip) -- 512 threads = 8 waves as 4 x 2, wave tile 64 x 32 NJ, ONE f32 accumulator
// acc[2][NJ] of v_mfma_f32_32x32x16_f16 fragments -- share
//   * the scratch layout (header of flags + error word, then one accumulator fragment per slot) and the LDS row swizzle,
//   * the launch plans (gp_plan256.h, plain C++ that the launchers and the CPU tests run too): the hosts' decisions per launch, and the
//     slot plan -- which (tile, unit) ranges a workgroup runs and in which order (GpSlotPlan) -- with the slots-per-tile rules,
//   * the deterministic accumulator hand-over between the slots of a split tile (gp_handoff_wait, gp_frag_publish / _load / _add),
//   * the three-product matrix step (gp_mfma3_step) and the loop of two wave groups half a step apart (gp_two_group_loop),
//   * the packed plane arithmetic of the tile epilogues (gp_hi_pair, gp_lo_pair, gp_sum_planes, gp_absmax3).
// Device code only but for gp_plan256.h; everything is inlined into the kernels (they sit at the register limit: a call would spill).
#pragma once
#include "gp_common.h"
#include "gp_plan256.h"  // kSlots, GpSlotPlan, the slots-per-tile rules, the hosts' launch plans
static_assert(kPlanEpiScaleRes == GP_EPI_BIAS_I_SCALE_RES && kPlanEpiGeluPlanes == GP_EPI_GELU_PLANES && kPlanEpiBiasPlanes == GP_EPI_BIAS_I_PLANES,
              "gp_plan256.h names the epilogues of the tile-shape policy by their C-ABI numbers");

typedef _Float16 gp_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int gp_u32x4 __attribute__((ext_vector_type(4)));

// ---- scratch: [flags: one int per slot .. error word .. padded to kHeaderBytes][kSlots accumulator fragments of kFragFloats].  A forward
// shares ONE scratch between these kernels and gp_gemm.hip's stream-K, so the header sizes must agree and this family's error word lies
// beyond the stream-K flags and their error word (flags[kGpSkMaxSlots]).
constexpr int kTileThreads = 512;                  // threads of a workgroup: 8 waves
constexpr int kErrWord = 1025;                     // header word set when a hand-over timed out
constexpr size_t kHeaderBytes = 8192;
constexpr size_t kFragFloats = (size_t)256 * 256;  // f32 accumulators of a 256 x 256 tile
constexpr int kSpin = 400000;                      // x ~0.4 us: a lost hand-off ends in an error word, never in a hang
constexpr unsigned kOob = 0x80000000u;             // buffer offset beyond every plane: the load returns zeros
constexpr int kRowHalfs = 32;                      // halfs per LDS operand row: one k-step = 64 bytes = four 16-byte chunks
static_assert(kHeaderBytes == kGpSkHeaderBytes, "one scratch serves gp_gemm.hip's stream-K and the 256-tile kernels: same header");
static_assert(kErrWord > kGpSkMaxSlots && (size_t)(kErrWord + 1) * sizeof(int) <= kHeaderBytes,
              "the error word lies beyond the stream-K flags + error word and inside the header");

// 64-byte LDS rows, the 16-byte chunk kc of a row XOR-placed by row bits 2-3 (offset in halfs): the 32 rows x 2 chunks of a fragment read
// and the 4 chunks x 16 rows of a staging write are both conflict-free.
__device__ __forceinline__ int gp_swz(int row, int kc) { return row * kRowHalfs + ((kc ^ ((row >> 2) & 3)) << 3); }

// ---- Hand-over.  A flag is valid when it holds THIS launch's epoch (no reset between launches).  One lane waits for the flags of slots
// first_slot, first_slot - stride, .. last_slot (nearest first; first_slot == last_slot: the one flag of the serial hand-over), sleeping
// between polls; after kSpin polls it sets the scratch's error word and the status bit and goes on (the tile is garbage, nothing hangs).
// Then an agent-scope acquire and the workgroup's barrier: every thread may read the fragments.
// Precondition: first_slot and last_slot lie on the same lattice of `stride` and first_slot >= last_slot - stride; the number of flags is
// (first_slot - last_slot) / stride + 1, so first_slot == last_slot - stride (a parallel split of S = 1) waits for none.
__device__ __forceinline__ void gp_handoff_wait(int* flags, int first_slot, int last_slot, int stride, int epoch, int* status)
{
    if (threadIdx.x == 0) {
        const int count = (first_slot - last_slot) / stride + 1;  // (a constant 1 for the single flag: no loop is left)
        for (int i = 0, m = first_slot; i < count; ++i, m -= stride) {
            int spins = 0;
            while (__hip_atomic_load(flags + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
                __builtin_amdgcn_s_sleep(16);
                if (++spins > kSpin) {
                    __hip_atomic_store(flags + kErrWord, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    gp_raise(status, GP_ST_HANDOFF_SPLIT);
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

// An accumulator fragment in the scratch: 16-byte piece q = (mi * 4 + ni) * 4 + r4 of thread tid at [q][tid] (a wave instruction covers
// 1 KB contiguous), moved by buffer accesses: one 32-bit lane offset + a scalar offset per piece.  (The first form, thread-major through
// 64-bit flat addresses 8 KB apart, cost an address pair per piece: 100 spilled registers in gemm_planes256_kernel.)  A fragment is
// written and read inside one launch by the same kernel: the layout is invisible outside.
// The casts are whole-vector: element-wise __builtin_bit_cast of vector lanes miscompiles (every r4 got lane group 0).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gp_frag_rsrc(float* partial, int slot)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)(partial + (size_t)slot * kFragFloats), 0, (int)(kFragFloats * sizeof(float)), 0x00020000);
}
// (stride 4 per mi for EVERY NJ, as the convolution kernels had it: NJ < 4 leaves holes in the slot's 32 piece rows; the plane GEMM's
// 256 x 128 builds used (mi * NJ + ni) * 4 + r4 before -- same pieces, other scratch offsets)
constexpr unsigned gp_frag_piece(int mi, int ni, int r4) { return (unsigned)(((mi * 4 + ni) * 4 + r4) * kTileThreads) * 16u; }

// Publishes acc as the fragment of `slot` (agent-scope release by one lane).  publish_flag = false: the fragment is written but never
// announced -- the probe build's LOST hand-off, after which the waiter must time out and flag it.
template <int NJ>
__device__ __forceinline__ void gp_frag_publish(const f32x16 (&acc)[2][NJ], float* partial, int slot, int* flags, int epoch, bool publish_flag)
{
    const __amdgpu_buffer_rsrc_t rf = gp_frag_rsrc(partial, slot);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NJ; ++ni)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                f32x4 vf;
                vf[0] = acc[mi][ni][r4 * 4 + 0]; vf[1] = acc[mi][ni][r4 * 4 + 1];
                vf[2] = acc[mi][ni][r4 * 4 + 2]; vf[3] = acc[mi][ni][r4 * 4 + 3];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gp_u32x4, vf), rf, threadIdx.x * 16u, gp_frag_piece(mi, ni, r4), 0);
            }
    // (write-through `sc1` stores through inline asm, which the guide prices at 3.0 us against 8.2 us per 64 KB-per-workgroup
    // publish, measured 17 -> 14 us per 256 KB in the plane GEMM: all slots publish at once and the 48 MB are bandwidth -- not kept)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (publish_flag) __hip_atomic_store(flags + slot, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// (zeroing acc stays three loops in the kernels: through a helper the plane GEMM's parallel-split builds spilled 6 - 26 registers more)
// acc = the fragment of `slot` (the serial hand-over: a rest segment continues where the head stopped)
template <int NJ>
__device__ __forceinline__ void gp_frag_load(f32x16 (&acc)[2][NJ], float* partial, int slot)
{
    const __amdgpu_buffer_rsrc_t rf = gp_frag_rsrc(partial, slot);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NJ; ++ni)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 vf = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rf, threadIdx.x * 16u, gp_frag_piece(mi, ni, r4), 0));
                acc[mi][ni][r4 * 4 + 0] = vf[0]; acc[mi][ni][r4 * 4 + 1] = vf[1];
                acc[mi][ni][r4 * 4 + 2] = vf[2]; acc[mi][ni][r4 * 4 + 3] = vf[3];
            }
}

// acc += the fragment of `slot` (the parallel split), RQ 16-byte loads in flight per lane, then their 4 RQ adds
template <int NJ, int RQ>
__device__ __forceinline__ void gp_frag_add(f32x16 (&acc)[2][NJ], float* partial, int slot)
{
    static_assert((8 * NJ) % RQ == 0, "RQ divides the pieces of a fragment");
    const __amdgpu_buffer_rsrc_t rf = gp_frag_rsrc(partial, slot);
#pragma unroll
    for (int q0 = 0; q0 < 8 * NJ; q0 += RQ) {
        gp_u32x4 v[RQ];
#pragma unroll
        for (int u = 0; u < RQ; ++u) {
            const int f = q0 + u;
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(rf, threadIdx.x * 16u, gp_frag_piece(f / (4 * NJ), (f >> 2) % NJ, f & 3), 0);
        }
#pragma unroll
        for (int u = 0; u < RQ; ++u) {
            const int f = q0 + u, mi = f / (4 * NJ), ni = (f >> 2) % NJ, r4 = f & 3;
            const f32x4 vf = __builtin_bit_cast(f32x4, v[u]);
            acc[mi][ni][r4 * 4 + 0] += vf[0]; acc[mi][ni][r4 * 4 + 1] += vf[1];
            acc[mi][ni][r4 * 4 + 2] += vf[2]; acc[mi][ni][r4 * 4 + 3] += vf[3];
        }
    }
}

// ---- The matrix phase of one k-step (32 k = two k16 blocks): per block the three products hi*hi + hi*lo + lo*hi into the ONE accumulator.
// Operand rows are 64-byte LDS rows (gp_swz); A fragment mi is at LA_hi / LA_lo + arow + a0[mi] (first k16 block) and + a1[mi] (second),
// B fragment ni at LB_hi / LB_lo + brow + ni * 32 rows + bk0 / bk1 (arow, brow: the lane's row; conv_halo_kernel's A rows differ per
// fragment and tap: all in a0 / a1).  Read and issue order:
//     ah bh bl al | ah*bh ah*bl | ch dh | al*bh | dl cl | ch*dh ch*dl cl*dh
// -- the second block's fragments replace the dead ones (ah, bl) under the MFMAs in flight.  Raised priority from before the fragment
// reads: they must not queue behind the other wave group's staging.
template <int NJ>
__device__ __forceinline__ void gp_mfma3_step(f32x16 (&acc)[2][NJ], const _Float16* LA_hi, const _Float16* LA_lo, int arow,
                                              const int (&a0)[2], const int (&a1)[2], const _Float16* LB_hi, const _Float16* LB_lo, int brow, int bk0, int bk1)
{
#define GP_MFMA(A_, B_, mi, ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A_[mi], B_[ni], acc[mi][ni], 0, 0, 0)
    __builtin_amdgcn_s_setprio(1);
    gp_f16x8 ah[2], al[2], bh[NJ], bl[NJ], ch[2], cl[2], dh[NJ], dl[NJ];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) ah[mi] = *reinterpret_cast<const gp_f16x8*>(LA_hi + arow + a0[mi]);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) bh[ni] = *reinterpret_cast<const gp_f16x8*>(LB_hi + brow + ni * 32 * kRowHalfs + bk0);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) bl[ni] = *reinterpret_cast<const gp_f16x8*>(LB_lo + brow + ni * 32 * kRowHalfs + bk0);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) al[mi] = *reinterpret_cast<const gp_f16x8*>(LA_lo + arow + a0[mi]);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) { GP_MFMA(ah, bh, 0, ni); GP_MFMA(ah, bh, 1, ni); }
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) { GP_MFMA(ah, bl, 0, ni); GP_MFMA(ah, bl, 1, ni); }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) ch[mi] = *reinterpret_cast<const gp_f16x8*>(LA_hi + arow + a1[mi]);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) dh[ni] = *reinterpret_cast<const gp_f16x8*>(LB_hi + brow + ni * 32 * kRowHalfs + bk1);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) { GP_MFMA(al, bh, 0, ni); GP_MFMA(al, bh, 1, ni); }
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) dl[ni] = *reinterpret_cast<const gp_f16x8*>(LB_lo + brow + ni * 32 * kRowHalfs + bk1);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) cl[mi] = *reinterpret_cast<const gp_f16x8*>(LA_lo + arow + a1[mi]);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) { GP_MFMA(ch, dh, 0, ni); GP_MFMA(ch, dh, 1, ni); }
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) { GP_MFMA(ch, dl, 0, ni); GP_MFMA(ch, dl, 1, ni); }
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni) { GP_MFMA(cl, dh, 0, ni); GP_MFMA(cl, dh, 1, ni); }
    __builtin_amdgcn_s_setprio(0);
#undef GP_MFMA
}

// ---- One loop body for both wave groups (grp = wave >> 2; one wave of each per SIMD): while one group issues the MFMAs of slab s
// (matrix phase c_phase(s)) the other writes its share of slab s + 1 to LDS and issues its loads of slab s + 2 (memory phase
// m_phase(s + 1)); waves 4-7 run one memory phase ahead.  ONE barrier per k-step (ns - 1 for every wave); what it orders: C(s+1)
// after every wave's M(s+1), M(s+2) after every wave's C(s):
//     waves 0-3:  C0 M1 | C1 M2 | ...          waves 4-7:  M1 C0 | M2 C1 | ...
// After a barrier waves 0-3 start their MFMAs at once and waves 4-7 stage first, so the offset is kept by the code
// order; the matrix phases overlap in part (the pipe is shared, its work per step is the same).  Measured on the
// fc2 shape (profiles/r01_probe_planes256_variants.txt): strict alternation with two barriers per step 4170
// cycles per step, this 3670 (matrix pipe 84 % busy in-loop), without the matrix-phase priority 3850.
// after_c / after_m: called behind the barrier that may follow each phase (the time stamps of the plane GEMM's TIMING builds).
struct GpNoHook {
    __device__ __forceinline__ void operator()() const {}
};
template <class CPhase, class MPhase, class AfterC = GpNoHook, class AfterM = GpNoHook>
__device__ __forceinline__ void gp_two_group_loop(int ns, int grp, CPhase c_phase, MPhase m_phase, AfterC after_c = AfterC(), AfterM after_m = AfterM())
{
    if (grp) m_phase(1);
    for (int s = 0; s < ns; ++s) {
        c_phase(s);
        if (grp && s + 1 < ns) __syncthreads();
        after_c();
        m_phase(s + 1 + grp);
        if (!grp && s + 1 < ns) __syncthreads();
        after_m();
    }
}

// ---- Thin plane arithmetic of the tile epilogues and attention (round 4).  The round-3 segment probes put the arithmetic half of a plane
// epilogue at 8.5 vector instructions per element (readlane + select for the bias, multiply, add, x 8, two conversions, a subtraction, a
// third conversion, a compare) and showed that it adds to the matrix work instead of hiding behind it.  Here a pair of values becomes its
// two f16 planes in three instructions (v_cvt_pk_f16_f32; v_fma_mixlo / mixhi_f16 computing v - hi with the f16 operand read straight
// from the packed hi pair), and the range guard is a NaN-propagating v_maximum3_f32 over |v| per pair.
__device__ __forceinline__ unsigned gp_hi_pair(float v0, float v1)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 h;
    h[0] = (_Float16)v0;
    h[1] = (_Float16)v1;
    return __builtin_bit_cast(unsigned, h);
}
// (f16(v0 - hi.lo), f16(v1 - hi.hi)) in one register.  v - hi is exact in f32 (hi = v rounded to 11 bits), so the single rounding
// of the mixed-precision fma equals the f32 subtraction + conversion the other plane producers use.
__device__ __forceinline__ unsigned gp_lo_pair(float v0, float v1, unsigned hi)
{
    unsigned lo;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(lo)
        : "v"(v0), "v"(v1), "v"(hi));
    return lo;
}
// (float)h + (float)l of the f16 halves HALF of two plane words -- exact in f32 -- as ONE v_fma_mix_f32 reading both halves in place
template <int HALF>
__device__ __forceinline__ float gp_sum_planes(unsigned h, unsigned l)
{
    float r;
    if (HALF == 0) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "v"(l));
    else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "v"(l));
    return r;
}
__device__ __forceinline__ float gp_absmax3(float m, float v0, float v1)  // v_maximum3_f32: a NaN operand makes the result NaN
{
    return __builtin_elementwise_maximum(m, __builtin_elementwise_maximum(__builtin_fabsf(v0), __builtin_fabsf(v1)));
}
