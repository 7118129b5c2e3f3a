// The launch plans of the 256-tile kernels (gp_tile256.h), stated ONCE in plain C++17: no HIP include, no HIP type.  Three readers run
// this text: the launchers (gp_split256.hip, gp_conv256.hip: the host decisions), the kernels (GpSlotPlan and the slots-per-tile rules,
// inlined) and the CPU tests (gp_plan256_c.cpp wraps it for ctypes: gigapose_testing/plan256.py).
//   Host: gp_split256_usable, gp_planes256_plan (usable, ragged strip, tile shape, cap on slots per tile, which build),
//         gp_conv256_plan / gp_stem256_plan (refused or not, kernel, tile counts, units, parallel or serial, slots per XCD, cap).
//   Device: GpSlotPlan (the segments of one slot), gp_planes_par_slots / gp_halo_par_slots (slots per tile of a parallel split).
#pragma once

#ifdef __HIPCC__
#define GP_PLAN_FN __host__ __device__ __forceinline__
#else
#define GP_PLAN_FN inline
#endif

constexpr int kSlots = 256;                     // workgroups of a full launch: one per CU
constexpr int kPlanTile = 256, kPlanK = 32;     // rows (and full-width columns) of a tile; k per k-step = input channels per channel block
// the epilogue codes (gp_common.h: GpEpilogue; C ABI) the plane GEMM's tile-shape policy names; gp_tile256.h holds them to the enum
constexpr int kPlanEpiScaleRes = 3, kPlanEpiGeluPlanes = 6, kPlanEpiBiasPlanes = 7;

GP_PLAN_FN constexpr int gp_plan_max(int a, int b) { return a > b ? a : b; }
GP_PLAN_FN constexpr int gp_plan_min(int a, int b) { return a < b ? a : b; }

// ---- Slot plan.  Workgroup p of the grid is slot n = p >> 3 of XCD x = p & 7 (the hardware places block id on XCD id % 8); each XCD
// owns one contiguous chunk of the tile list (n_t tiles from t_lo) and its slots_x slots cut that chunk's (tile, unit) space -- a unit is
// a k-step, or a block of 32 input channels in conv_halo_kernel -- into segments: whole tiles, at most one HEAD (the first units of a
// tile: its accumulator fragment is published for the slot that continues the tile) and at most one REST (continues a tile).
//   Data-parallel rounds first: while the chunk holds two or more tiles per slot, round r gives slot n the whole tile
// r * slots_x + n -- the 32 slots of an XCD then sit on the same k-step of 32 neighbouring tiles (4 i-panels x 8
// j-panels) and share their operand slabs in that XCD's L2.  Only the last round + remainder is cut stream-K style
// (its slots run at staggered k offsets and get no L2 reuse: 1.9 GB fetched per fc1 launch when everything was).
//   PAR (par_S > 0; fewer tiles than slots): S = par_S slots per tile, each an equal share of the tile's units from a zero accumulator,
// all at once; slot n holds part n % S of tile n / S, slots beyond S * tiles have no tile.  All but the last publish their partial
// accumulator (heads), the slot holding the last range (a rest) adds them in slot order, nearest first -- a fixed order, the result
// depends on the shape only -- and runs the epilogue.  S = 1: whole tiles, no exchange.  (The serial hand-over, par_S = 0, keeps a split
// tile's summation order but makes its slots wait for each other: with fewer tiles than slots every tile is split and a launch would
// take as long as one whole tile.)
struct GpSlotPlan {
    struct Segment {
        int tile;      // index into the launch's tile list
        int u0, u1;    // units [u0, u1) of that tile
        bool is_head;  // publishes its accumulator instead of running the epilogue
        bool is_rest;  // continues a tile: takes over (par_S = 0) or adds (par_S > 0) the fragments of the slots before it
    };
    int p, x, n, slots_x;
    int upt, t_lo, rounds_dp, n_dp, ta, sa, tb, sb, n_head, n_rest, first_whole, n_seg;

    // slot, grid: the kernels pass blockIdx.x and gridDim.x
    GP_PLAN_FN GpSlotPlan(unsigned slot, unsigned grid, int tiles, int units_per_tile, bool dp_rounds_allowed, int par_S)
    {
        p = slot, x = p & 7, n = p >> 3, slots_x = grid >> 3;
        upt = units_per_tile;
        t_lo = (int)((long long)tiles * x / 8);
        const int n_t = (int)((long long)tiles * (x + 1) / 8) - t_lo;
        rounds_dp = (dp_rounds_allowed && n_t / slots_x > 1) ? n_t / slots_x - 1 : 0;
        n_dp = rounds_dp * slots_x;
        const long long U = (long long)(n_t - n_dp) * upt;
        long long u0 = U * n / slots_x, u1 = U * (n + 1) / slots_x;
        if (par_S > 0) {
            const int tile = n / par_S, part = n - tile * par_S;
            u0 = u1 = 0;
            if (tile < n_t) {
                u0 = (long long)tile * upt + upt * part / par_S;
                u1 = (long long)tile * upt + upt * (part + 1) / par_S;
            }
        }
        ta = (int)(u0 / upt), sa = (int)(u0 % upt);
        tb = (int)(u1 / upt), sb = (int)(u1 % upt);
        n_head = sb > 0 ? 1 : 0, n_rest = sa > 0 ? 1 : 0;
        first_whole = ta + n_rest;
        n_seg = rounds_dp + n_head + (tb - first_whole) + n_rest;
    }
    // tiles of XCD x's chunk (the cap of PAR's slots per tile is slots_x / tiles of the slot's own chunk)
    static GP_PLAN_FN int chunk_tiles(int tiles, int x)
    {
        return (int)((long long)tiles * (x + 1) / 8) - (int)((long long)tiles * x / 8);
    }
    // order: data-parallel rounds, the head, whole tiles, the rest
    GP_PLAN_FN Segment segment(int seg) const
    {
        const bool is_dp = seg < rounds_dp;
        const bool is_head = !is_dp && seg - rounds_dp < n_head;
        const bool is_rest = !is_dp && n_rest && seg == n_seg - 1;
        const int t = is_dp ? seg * slots_x + n : n_dp + (is_head ? tb : (is_rest ? ta : first_whole + seg - rounds_dp - n_head));
        return {t_lo + t, is_rest ? sa : 0, is_head ? sb : upt, is_head, is_rest};
    }
};

// Slots per tile of a parallel split, per XCD (chunk_tiles: GpSlotPlan::chunk_tiles of the slot's XCD).
// The plane GEMM: floor(slots / tiles) of the chunk, at most the host's cap (k-steps per slot: gp_planes256_plan's par).
GP_PLAN_FN int gp_planes_par_slots(int cap, int slots_x, int chunk_tiles)
{
    return gp_plan_max(1, gp_plan_min(cap, slots_x / gp_plan_max(chunk_tiles, 1)));
}
// The halo convolution: no more than the tile has channel blocks (ncb) and at most the host's cap (gp_conv256_plan's par_cap).
GP_PLAN_FN int gp_halo_par_slots(int par_cap, int slots_x, int chunk_tiles, int ncb)
{
    return gp_plan_min(gp_plan_min(gp_plan_max(1, slots_x / gp_plan_max(chunk_tiles, 1)), ncb), gp_plan_max(1, par_cap));
}
// Which plane-GEMM builds add partial accumulators at all: the GELU build keeps whole tiles (S = 1) in every PAR build, the
// PSPLIT = false builds have the reduction compiled out (gemm_planes256_kernel)
GP_PLAN_FN constexpr bool gp_planes_build_splits(bool par, bool psplit, int epilogue) { return par && psplit && epilogue != kPlanEpiGeluPlanes; }

// ---- The probe hooks (A/B switches of the -DGP_PROBES library; the product never changes the defaults).  Each launcher file keeps one
// instance and reads its own fields.
// A tile is split over at most K / 32 / kParMinSteps slots: below 16 k-steps per slot the partial accumulators (256 KB each, published by
// all non-owners at once, then read by the owner) cost more than the shorter k loop saves -- proj (K = 1024) at 16 crops 69 -> 62 us with
// two instead of four slots per tile, at 8 crops 74 -> 55 us with two or four instead of eight (PAR_MIN_STEPS=.. tools/probe_planes_timeline.py).
constexpr int kParMinSteps = 16;
struct GpPlanHooks {
    int planes_dp = 1;                        // bit 0: data-parallel rounds before the stream-K remainder (0: everything stream-K); bit 1: test hook, head fragments are never published
    int planes_par = 1;                       // 0: shapes with fewer tiles than slots are refused (the caller falls back to the 128 x 128 kernel)
    int planes_half = 1;                      // 0: never the 256 x 128 tiles
    int planes_par_min_steps = kParMinSteps;  // k-steps per slot of a split tile at least
    int conv_halo = 1;                        // 3 x 3 / stride 1 layers take the halo kernel
    int conv_par = 1;                         // ... and its parallel split below 256 tiles
    int conv_par_min_cb = 1;                  // channel blocks (9 k-steps each) per slot of a split tile at least
};

// ---- gemm_split256_kernel: whole 256 x 256 tiles, at least one per slot
GP_PLAN_FN bool gp_split256_usable(int I, int J, int K)
{
    return I % kPlanTile == 0 && J % kPlanTile == 0 && K % kPlanK == 0 && (long long)(I / kPlanTile) * (J / kPlanTile) >= kSlots;
}

// ---- gemm_planes256_kernel.  J_valid <= J: rows of B that carry data (J itself stays a multiple of 256: the buffers are padded).
// Tiles cover floor(J_valid / 256) * 256 rows (J_main), strip_phase the rest in strip_fj fragments of 32 rows (rows beyond
// round_up(J_valid, 32) are neither read nor written).
enum GpPlanesBuild {
    GP_PLANES_SERIAL = 0,     // gemm_planes256_kernel<EPI>: at least one tile per slot, data-parallel rounds + serial hand-over
    GP_PLANES_PAR = 1,        // <EPI, .., PAR = true>: fewer tiles than slots, parallel split-K
    GP_PLANES_PAR_HALF = 2,   // <EPI, .., true, NJ = 2>: the same on 256 x 128 tiles
    GP_PLANES_PAR_WHOLE = 3,  // <EPI, .., true, 4, PSPLIT = false>: 129-255 whole tiles, one per slot
};
struct GpPlanesPlan {
    bool usable;             // false: the entry point refuses the shape (the other fields are then not to be used)
    int J_main, strip_fj;
    int tiles_i, tiles_j;    // tiles_j counts tiles of the build's width: 256 columns, 128 for GP_PLANES_PAR_HALF
    int par;                 // 0: serial; else the cap on slots per tile (gp_planes_par_slots)
    int build;               // GpPlanesBuild
    bool splits;             // the build adds partial accumulators (gp_planes_build_splits); false: every tile whole on one slot
};
// Fewer tiles than slots (B < 64 crops at ViT-L): the kernel's parallel split-K mode needs at least one tile per XCD and one
// k-step per slot (every slot's range then lies inside one or two tiles).
GP_PLAN_FN bool gp_planes_par_usable(int I, int J_main, int K)
{
    if (I <= 0 || J_main <= 0 || I % kPlanTile || J_main % kPlanTile || K % kPlanK) return false;
    const long long T = (long long)(I / kPlanTile) * (J_main / kPlanTile);
    return T < kSlots && T >= 8 && (T / 8) * (K / kPlanK) >= kSlots / 8;
}
GP_PLAN_FN int gp_planes_par_cap(const GpPlanHooks& h, int K) { return gp_plan_max(1, (K / kPlanK) / h.planes_par_min_steps); }
// traced: the time-stamped probe builds exist for the 256 x 256 serial and parallel-split kernels only
GP_PLAN_FN GpPlanesPlan gp_planes256_plan(const GpPlanHooks& h, int I, int J, int J_valid, int K, int epilogue, bool traced = false)
{
    GpPlanesPlan pl{};
    pl.J_main = (J_valid >= J || J_valid <= 0) ? J : (J_valid / kPlanTile) * kPlanTile;
    pl.strip_fj = (pl.J_main == J) ? 0 : (J_valid - pl.J_main + 31) / 32;
    pl.usable = !(J % kPlanTile || J_valid > J) &&
                !((long long)(I / 32) * pl.strip_fj + kSlots >= 4096) &&  // strip fragments must fit the 12-bit counter (strip_grab)
                (gp_split256_usable(I, pl.J_main, K) || (h.planes_par && gp_planes_par_usable(I, pl.J_main, K)));
    pl.tiles_i = I / kPlanTile, pl.tiles_j = pl.J_main / kPlanTile;
    const long long T256 = (long long)pl.tiles_i * pl.tiles_j;
    pl.par = T256 < kSlots ? gp_planes_par_cap(h, K) : 0;
    const bool epi_half = epilogue == kPlanEpiScaleRes || epilogue == kPlanEpiGeluPlanes || epilogue == kPlanEpiBiasPlanes;
    // 256 x 128 tiles where the 256 x 256 ones fill at most half the slots (ViT-L below ~16 crops): the parallel split-K build on twice
    // the tiles -- proj / fc2 split every tile over half as many slots with half-size partial accumulators, q|k|v and fc1 stop
    // splitting / fill the chip with whole tiles.  (Between 128 and 256 whole tiles, twice as many half-width tiles cut stream-K
    // style over all slots by the serial hand-over build was measured too: ViT-L forward at 12 / 16 / 40 / 48 crops 8.55 -> 8.95,
    // 10.39 -> 10.44, 22.95 -> 22.5, 25.19 -> 25.55 ms -- the hand-overs cost what the balance gains; not kept.)
    if (pl.par && !traced && h.planes_half && epi_half && 2 * T256 <= kSlots) {
        pl.build = GP_PLANES_PAR_HALF;
        pl.tiles_j = pl.J_main / (kPlanTile / 2);
    } else if (pl.par && !traced && 2 * T256 > kSlots && (epilogue == kPlanEpiScaleRes || epilogue == kPlanEpiBiasPlanes)) {
        // 129-255 whole tiles, one per slot (S = floor(256 / tiles) = 1): the PAR build WITHOUT the split-K reduction.  With the 256 x 128
        // tiles taking every launch of at most 128 tiles, the 256 x 256 PAR build only ever runs 129-255 WHOLE tiles (ViT-L: q|k|v at
        // 11-21 crops, proj / fc2 at 33-63) -- yet it carried the reduction's registers (gemm_planes256_kernel: PSPLIT)
        pl.build = GP_PLANES_PAR_WHOLE;
        pl.par = 1;
    } else {
        // fewer tiles than slots: the parallel split-K build (its own instantiation: the serial hand-over kernel keeps its registers)
        pl.build = pl.par ? GP_PLANES_PAR : GP_PLANES_SERIAL;
    }
    pl.splits = gp_planes_build_splits(pl.build == GP_PLANES_PAR || pl.build == GP_PLANES_PAR_HALF, true, epilogue);
    return pl;
}

// ---- conv_planes_kernel (gather; the stem) and conv_halo_kernel: tile 256 pixels x 64 ni output channels
enum GpConvKernel { GP_CONV_GATHER = 0, GP_CONV_HALO = 1, GP_CONV_STEM = 2 };
enum GpConvRefusal { GP_CONV_OK = 0, GP_CONV_BAD_SIZES = 1, GP_CONV_BAD_CHANNELS = 2, GP_CONV_BAD_PIXELS = 3 };
struct GpConvPlan {
    int refused;                // GpConvRefusal: the first shape rule of the entry point that fails (the other fields are then not to be used)
    int kernel;                 // GpConvKernel
    int ni;                     // 64-channel fragments per tile: 128 -> 2, 192 -> 3, >= 256 -> 4
    int tiles_i, tiles_j;
    int upt, steps_per_unit;    // units per tile (k-steps; channel blocks of 9 k-steps in the halo kernel)
    bool par;                   // conv_halo_kernel<.., PAR = true>
    int slots_x;                // slots per XCD: the grid is 8 slots_x
    int par_cap;                // most slots a tile is split over (gp_halo_par_slots)
};
// Slots: all 256 CUs unless there are fewer tiles than slots AND so little work that cutting tiles would leave a slot with under 32
// k-steps per hand-over (the 1 x 1 head: 64 tiles x 16 steps -> 32 slots of two whole tiles).  A parallel split keeps every slot.
GP_PLAN_FN int gp_conv_slots_x(bool par, long long n_tiles, long long k_steps)
{
    int slots_x = 32;
    while (!par && slots_x > 1 && n_tiles < 8 * slots_x && k_steps / (8 * slots_x) < 32) slots_x >>= 1;
    return slots_x;
}
GP_PLAN_FN GpConvPlan gp_conv256_plan(const GpPlanHooks& h, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad)
{
    GpConvPlan pl{};
    pl.refused = GP_CONV_BAD_SIZES;
    if (!(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0)) return pl;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    const int K = KH * KW * Cin;
    const long long npix = (long long)B * OH * OW;
    pl.refused = GP_CONV_BAD_CHANNELS;
    if (!(Cin % 32 == 0 && Cout % 64 == 0 && KH * KW <= 9)) return pl;
    pl.refused = GP_CONV_BAD_PIXELS;
    if (!(npix % kPlanTile == 0)) return pl;
    pl.refused = GP_CONV_OK;
    pl.ni = Cout >= 256 ? 4 : Cout / 64;  // 128 -> 2, 192 -> 3, >= 256 -> 4
    pl.tiles_j = (Cout + 64 * pl.ni - 1) / (64 * pl.ni);
    pl.par_cap = 1;
    // 3 x 3 / stride 1 / pad 1 on 16 x 16 pixel blocks with the halo resident in LDS (conv_halo_kernel).  Needs H, W multiples of 16.
    if (h.conv_halo && KH == 3 && KW == 3 && stride == 1 && pad == 1 && H % 16 == 0 && W % 16 == 0 && Cin % 32 == 0 && Cout % 64 == 0) {
        pl.kernel = GP_CONV_HALO;
        pl.tiles_i = B * (OH / 16) * (OW / 16);
        const int ncb = Cin / kPlanK;
        pl.upt = ncb, pl.steps_per_unit = 9;
        const long long n_tiles = (long long)pl.tiles_i * pl.tiles_j, units = n_tiles * ncb * 9;
        pl.par = h.conv_par && n_tiles < 8 * 32 && n_tiles >= 8 && ncb >= 2;  // fewer tiles than slots: parallel split over channel blocks
        pl.par_cap = gp_plan_max(1, ncb / h.conv_par_min_cb);
        pl.slots_x = gp_conv_slots_x(pl.par, n_tiles, units);
        return pl;
    }
    pl.kernel = GP_CONV_GATHER;
    pl.tiles_i = (int)(npix / kPlanTile);
    pl.upt = K / kPlanK, pl.steps_per_unit = 1;
    const long long n_tiles = (long long)pl.tiles_i * pl.tiles_j, units = n_tiles * (K / kPlanK);
    pl.slots_x = gp_conv_slots_x(false, n_tiles, units);
    return pl;
}
// The 7 x 7 / stride 2 stem on S x S crops: conv_planes_kernel on all 256 slots, one kernel row (K = 7 x 32) per k-step
GP_PLAN_FN GpConvPlan gp_stem256_plan(int B, int S, int Cout)
{
    GpConvPlan pl{};
    pl.refused = GP_CONV_BAD_SIZES;
    if (!(B > 0 && S > 0 && S % 2 == 0 && Cout > 0 && (Cout == 128 || Cout == 192 || Cout % 256 == 0))) return pl;
    const long long npix = (long long)B * (S / 2) * (S / 2);
    pl.refused = GP_CONV_BAD_PIXELS;
    if (!(npix % kPlanTile == 0)) return pl;
    pl.refused = GP_CONV_OK;
    pl.kernel = GP_CONV_STEM;
    pl.ni = Cout >= 256 ? 4 : Cout / 64;
    pl.tiles_i = (int)(npix / kPlanTile);
    pl.tiles_j = (Cout + 64 * pl.ni - 1) / (64 * pl.ni);
    pl.upt = 7, pl.steps_per_unit = 1;
    pl.slots_x = 32, pl.par_cap = 1;
    return pl;
}
