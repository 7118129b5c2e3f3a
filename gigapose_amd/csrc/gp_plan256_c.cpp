// C wrapper of gp_plan256.h for the CPU tests (gigapose_testing/plan256.py loads it by ctypes): the SAME text the launchers and the
// kernels run, compiled by the host C++ compiler alone -- no HIP, no GPU.  Not part of the product libraries.
// hooks: null = the defaults, else the seven ints of GpPlanHooks in declaration order.  Results are written as ints in field order.
#include "gp_plan256.h"

static GpPlanHooks hooks_of(const int* h)
{
    GpPlanHooks g;
    if (h) g = GpPlanHooks{h[0], h[1], h[2], h[3], h[4], h[5], h[6]};
    return g;
}
static void conv_out(const GpConvPlan& p, int* out)
{
    const int v[10] = {p.refused, p.kernel, p.ni, p.tiles_i, p.tiles_j, p.upt, p.steps_per_unit, p.par, p.slots_x, p.par_cap};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}

extern "C" {

int gp_plan_split256_usable(int I, int J, int K) { return gp_split256_usable(I, J, K); }

// out[8]: usable, J_main, strip_fj, tiles_i, tiles_j, par, build, splits
void gp_plan_planes256(const int* hooks, int I, int J, int J_valid, int K, int epilogue, int traced, int* out)
{
    const GpPlanesPlan p = gp_planes256_plan(hooks_of(hooks), I, J, J_valid, K, epilogue, traced != 0);
    const int v[8] = {p.usable, p.J_main, p.strip_fj, p.tiles_i, p.tiles_j, p.par, p.build, p.splits};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}
int gp_plan_planes_par_cap(const int* hooks, int K) { return gp_planes_par_cap(hooks_of(hooks), K); }

// out[10]: refused, kernel, ni, tiles_i, tiles_j, upt, steps_per_unit, par, slots_x, par_cap
void gp_plan_conv256(const int* hooks, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* out)
{
    conv_out(gp_conv256_plan(hooks_of(hooks), B, H, W, Cin, Cout, KH, KW, stride, pad), out);
}
void gp_plan_stem256(int B, int S, int Cout, int* out) { conv_out(gp_stem256_plan(B, S, Cout), out); }

int gp_plan_chunk_tiles(int tiles, int x) { return GpSlotPlan::chunk_tiles(tiles, x); }
int gp_plan_planes_par_slots(int cap, int slots_x, int chunk_tiles) { return gp_planes_par_slots(cap, slots_x, chunk_tiles); }
int gp_plan_halo_par_slots(int par_cap, int slots_x, int chunk_tiles, int ncb) { return gp_halo_par_slots(par_cap, slots_x, chunk_tiles, ncb); }

// The segments of slot p of a grid of `grid` workgroups, in the order the slot runs them: out[6 i ..] = tile, u0, u1, is_head, is_rest, and
// whether it is a data-parallel round (i < rounds_dp), of segment i < min(n_seg, cap); returns n_seg
int gp_plan_slot_segments(int p, int grid, int tiles, int units_per_tile, int dp_rounds_allowed, int par_S, int* out, int cap)
{
    const GpSlotPlan plan((unsigned)p, (unsigned)grid, tiles, units_per_tile, dp_rounds_allowed != 0, par_S);
    for (int i = 0; i < plan.n_seg && i < cap; ++i) {
        const GpSlotPlan::Segment s = plan.segment(i);
        const int v[6] = {s.tile, s.u0, s.u1, s.is_head, s.is_rest, i < plan.rounds_dp};
        for (int k = 0; k < 6; ++k) out[6 * i + k] = v[k];
    }
    return plan.n_seg;
}

}  // extern "C"
