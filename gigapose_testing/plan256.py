"""ctypes front-end of the launch plans of the 256-tile kernels -- TEST INFRASTRUCTURE ONLY.

gigapose_amd/csrc/gp_plan256.h states the plans once, in plain C++: the launchers of gp_split256.hip / gp_conv256.hip and their kernels run
that text, and so do the CPU tests, through gp_plan256_c.cpp built by the host C++ compiler into gigapose_amd/libgigapose_plan256.so (no
HIP, no GPU; built on demand like the C oracle).  The package never loads it."""
import ctypes
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gigapose_amd", "csrc")
_SO = os.path.join(os.path.dirname(_CSRC), "libgigapose_plan256.so")
_lib = None

PLANES_BUILDS = ("serial", "par", "par128", "par-whole")      # GpPlanesBuild
CONV_KERNELS = ("gather", "halo", "stem")                      # GpConvKernel
HOOKS = ("planes_dp", "planes_par", "planes_half", "planes_par_min_steps", "conv_halo", "conv_par", "conv_par_min_cb")   # GpPlanHooks
_PLANES_FIELDS = ("usable", "J_main", "strip_fj", "tiles_i", "tiles_j", "par", "build", "splits")
_CONV_FIELDS = ("refused", "kernel", "ni", "tiles_i", "tiles_j", "upt", "steps_per_unit", "par", "slots_x", "par_cap")


def lib():
    global _lib
    if _lib is None:
        srcs = [os.path.join(_CSRC, f) for f in ("gp_plan256.h", "gp_plan256_c.cpp")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(map(os.path.getmtime, srcs)):
            subprocess.run(["make", "-C", _CSRC, "../libgigapose_plan256.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = ctypes.CDLL(_SO)
    return _lib


def _hooks(hooks):
    """dict of GpPlanHooks fields that differ from the defaults -> the C argument (None: all defaults)"""
    if not hooks:
        return None
    assert set(hooks) <= set(HOOKS), hooks
    default = dict(zip(HOOKS, (1, 1, 1, 16, 1, 1, 1)))
    return (ctypes.c_int * 7)(*[hooks.get(k, default[k]) for k in HOOKS])


def split256_usable(I, J, K):
    return bool(lib().gp_plan_split256_usable(I, J, K))


def planes256(I, J, J_valid, K, epilogue, traced=False, hooks=None):
    """gp_planes256_plan -> dict(usable, J_main, strip_fj, tiles_i, tiles_j, par, build in PLANES_BUILDS, splits)"""
    out = (ctypes.c_int * 8)()
    lib().gp_plan_planes256(_hooks(hooks), I, J, J_valid, K, epilogue, int(traced), out)
    d = dict(zip(_PLANES_FIELDS, out))
    return dict(d, usable=bool(d["usable"]), splits=bool(d["splits"]), build=PLANES_BUILDS[d["build"]])


def planes_par_cap(K, hooks=None):
    return lib().gp_plan_planes_par_cap(_hooks(hooks), K)


def _conv(out):
    d = dict(zip(_CONV_FIELDS, out))
    return dict(d, par=bool(d["par"]), kernel=CONV_KERNELS[d["kernel"]])


def conv256(B, H, W, Cin, Cout, KH, KW, stride, pad, hooks=None):
    """gp_conv256_plan -> dict(refused (0: no), kernel in CONV_KERNELS, ni, tiles_i, tiles_j, upt, steps_per_unit, par, slots_x, par_cap)"""
    out = (ctypes.c_int * 10)()
    lib().gp_plan_conv256(_hooks(hooks), B, H, W, Cin, Cout, KH, KW, stride, pad, out)
    return _conv(out)


def stem256(B, S, Cout):
    out = (ctypes.c_int * 10)()
    lib().gp_plan_stem256(B, S, Cout, out)
    return _conv(out)


def chunk_tiles(tiles, x):
    return lib().gp_plan_chunk_tiles(tiles, x)


def planes_par_slots(cap, slots_x, chunk):
    return lib().gp_plan_planes_par_slots(cap, slots_x, chunk)


def halo_par_slots(par_cap, slots_x, chunk, ncb):
    return lib().gp_plan_halo_par_slots(par_cap, slots_x, chunk, ncb)


def slot_segments(p, grid, tiles, units_per_tile, dp_rounds_allowed, par_S):
    """GpSlotPlan of workgroup p of a grid of `grid` -> [(tile, u0, u1, is_head, is_rest, is_dp)] in the order the slot runs them
    (is_dp: a whole tile of a data-parallel round)."""
    cap = 64
    while True:
        out = (ctypes.c_int * (6 * cap))()
        n = lib().gp_plan_slot_segments(p, grid, tiles, units_per_tile, int(bool(dp_rounds_allowed)), par_S, out, cap)
        if n <= cap:
            return [tuple(out[6 * i:6 * i + 3]) + tuple(bool(v) for v in out[6 * i + 3:6 * i + 6]) for i in range(n)]
        cap = n
