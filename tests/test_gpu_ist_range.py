"""GPU: the IST ResNet's range guards and its wide-kernel fallback, end to end.

In split numerics the ResNet keeps its activations as f16 planes of 8 x: |8 x| <= 65504 (kSplitPlaneLimit).  A value beyond it makes the kernel
that writes the planes set status bit 16 (GP_ST_SPLIT_RANGE_CONV); GigaPose._widen_split_range then moves the ResNet to the two-accumulator
128 x 128 kernels (gp_conv2d_nhwc_split: planes hi + lo / 2048 of x itself, |x| <= 65504), rebuilds every template bank and runs again.

  A  every plane-writing epilogue of gp_conv256.hip raises bit 16 exactly at the limit -- conv_planes_kernel<2|3|4> (gather; whole tiles and
     a tile cut into k-ranges), conv_halo_kernel<2|3|4, serial | parallel>, the stem (resize_stem_planes_kernel, conv_planes_kernel with
     stem = 1) -- and the flag only reports: every in-range output of a flagged launch is still right; the f32 NCHW output has no limit;
  B  both kernel families against float64 with inputs from 1e-4 to the top of their range, bound PER OUTPUT c mag + floor
     (gigapose_testing/stage_refs.py: conv_range_reference; tests/test_stage_refs.py shows what the bound rejects);
  C  a checkpoint / a crop whose activations pass 8190 makes GigaPose fall back, and the fallen-back model equals one that was told
     ResNet.conv_kernel = "128" from the start;
  D  beyond 65504 the wide kernels raise bit 16 as well (conv_split_kernel's plane epilogue, gp_split_weights): GigaPoseHipError, never
     inf / NaN in a hi plane under a clean status word.

No planted value goes anywhere but through f16 conversions.  Stage-level cases run on both libraries (also_on_probe_binary)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from test_gpu_split import also_on_probe_binary, binary_name, planes8

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANGE_BIT = 16


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


@functools.lru_cache(maxsize=None)  # per library, zeroed once, as ResNet._conv_planes keeps it: hand-overs are tagged with a per-launch epoch
def _scratch(binary):
    lib = _lib.lib()
    nb = lib.gp_conv2d_planes_workspace_bytes()
    return torch.zeros((nb + 3) // 4, dtype=torch.float32, device=DEV), nb


def scratch():
    return _scratch(binary_name())


def device_planes(case):
    """The case's f32 arrays as x 8 / x 64 planes on the device (gp_split_planes)."""
    cout = case["cout"]
    x = planes8(torch.from_numpy(case["X"]).to(DEV))
    w = planes8(torch.from_numpy(np.ascontiguousarray(case["Wt"].transpose(0, 2, 3, 1).reshape(cout, -1))).to(DEV), 64.0)
    r = planes8(torch.from_numpy(case["R"]).to(DEV)) if case["R"] is not None else (None, None)
    return x, w, r


def launch_planes(case, planes, relu, out="planes"):
    """ONE gp_conv2d_planes launch -> (status word, (hi, lo) or None, f32 NCHW or None).  out = "planes": out_f32_nchw = NULL;
    "f32": out_hi = out_lo = NULL (the head's form)."""
    (xh, xl), (wh, wl), (rh, rl) = planes
    B, hw, _, cin = case["X"].shape
    cout, k, oh = case["cout"], case["Wt"].shape[2], case["oh"]
    ohi = olo = of32 = None
    if out == "planes":
        ohi = torch.full((B, oh, oh, cout), -7.0, dtype=torch.float16, device=DEV)
        olo = torch.full((B, oh, oh, cout), -7.0, dtype=torch.float16, device=DEV)
    else:
        of32 = torch.full((B, cout, oh, oh), -7.0, device=DEV)
    ta, tb = torch.from_numpy(case["alpha"]).to(DEV), torch.from_numpy(case["beta"]).to(DEV)
    ws, nb = scratch()
    assert _lib.take_status() == 0
    _lib.call("gp_conv2d_planes", _lib.ptr(xh), _lib.ptr(xl), _lib.ptr(wh), _lib.ptr(wl), _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(rh), _lib.ptr(rl),
              _lib.i(B), _lib.i(hw), _lib.i(hw), _lib.i(cin), _lib.i(cout), _lib.i(k), _lib.i(k), _lib.i(case["stride"]), _lib.i(case["pad"]),
              _lib.i(relu), _lib.ptr(ohi), _lib.ptr(olo), _lib.ptr(of32), _lib.ptr(ws), ctypes.c_size_t(nb), _lib.stream_ptr())
    torch.cuda.synchronize()
    return _lib.take_status(), (None if ohi is None else (ohi.cpu(), olo.cpu())), (None if of32 is None else of32.cpu().double())


def reference_of(case, planes, relu):
    """float64 reference + bound coefficient on the values the DEVICE planes hold."""
    (xh, xl), (wh, wl), (rh, rl) = planes
    cout, k = case["cout"], case["Wt"].shape[2]
    x = sr.planes_value(xh.cpu(), xl.cpu(), 8.0)
    w = sr.planes_value(wh.cpu(), wl.cpu(), 64.0).reshape(cout, k, k, -1).permute(0, 3, 1, 2).contiguous()
    r = None if rh is None else sr.planes_value(rh.cpu(), rl.cpu(), 8.0)
    return sr.conv_range_reference(x, w, case["alpha"], case["beta"], r, case["stride"], case["pad"], relu=bool(relu))


def planes_nchw(hl):
    return sr.planes_value(hl[0], hl[1], 8.0).permute(0, 3, 1, 2)


def check_in_range_outputs(tag, got, ref, floor):
    """Every output whose float64 value is inside the plane range meets part B's bound (the f32 output: every output)."""
    legal = (8.0 * ref["y"].abs() <= sr.F16_MAX) if floor is not None else torch.ones_like(ref["y"], dtype=torch.bool)
    worst, at = sr.conv_bound_worst(got, ref, floor, where=legal)
    print(f"    {tag}: c {ref['c']:.2e}, worst err / bound {worst:.3f} at {at} over {int(legal.sum())} of {legal.numel()} outputs")
    assert worst <= 1.0, (tag, worst, at)


ROUTE_DOC = {
    "gather_ni2": "32 -> 128, 3 x 3 stride 2 on 32 x 32, B = 1: stride 2 -> not the halo kernel (gp_conv256_plan); ni = 128 / 64 = 2 -> conv_planes_kernel<2>, one whole tile",
    "gather_ni3_1x1": "32 -> 192, 1 x 1 stride 2: ni = 3 -> conv_planes_kernel<3> (alpha | beta through the LDS stash), K = 32: ONE k-step",
    "gather_ni4_two_channel_tiles": "32 -> 512, 3 x 3 stride 2: ni = 4, tiles_j = 2 -> conv_planes_kernel<4>, two whole tiles on two XCD chunks",
    "gather_3x3_s1_not_16": "32 -> 128, 3 x 3 stride 1 on 8 x 8, B = 4: H % 16 != 0 -> the halo kernel refuses, conv_planes_kernel<2>",
    "gather_cut_tiles": "256 -> 512, 3 x 3 stride 2 on 32 x 32, B = 4: 8 tiles x 72 k-steps = 576 units -> slots_x = 2 (576 / 16 = 36 >= 32), one tile "
                        "per XCD chunk cut into two k-ranges: slot 0 publishes, slot 1 takes over and runs the epilogue (B = 1, 2, 3: slots_x = 1, whole tiles)",
    "halo_cout64": "32 -> 64, 3 x 3 stride 1 on 16 x 16, B = 1: ni = 64 / 64 = 1 -> the else branch, conv_halo_kernel<4, false>; 64 of its 256 columns valid",
    "halo_ni2_serial": "64 -> 128 on 16 x 16, B = 1: one tile (< 8) -> no parallel split, conv_halo_kernel<2, false>; two channel blocks (halo prefetch)",
    "halo_ni2_parallel": "64 -> 128 on 16 x 16, B = 8: 8 tiles (8 <= tiles < 256), 2 channel blocks -> conv_halo_kernel<2, true>: the slot of the last range adds and finishes",
    "halo_ni3_parallel": "64 -> 192, B = 8 -> conv_halo_kernel<3, true>",
    "halo_ni4_parallel": "64 -> 256, B = 8 -> conv_halo_kernel<4, true>",
}
assert set(ROUTE_DOC) == set(sr.CONV_GUARD_ROUTES)


# ---------------------------------------------------------------------------------------------------------------- A: the guards of gp_conv2d_planes
@also_on_probe_binary
@pytest.mark.parametrize("route", list(sr.CONV_GUARD_ROUTES))
def test_conv_planes_guard_zero_weight_channel(route):
    """Which kernel a route reaches and why: ROUTE_DOC[route] (printed).  One output channel has zero weights, alpha = 1, beta = v: its value is v
    exactly.  v = 8188 -> 8 v = 65504, the largest finite f16: status 0 and hi + lo == 65504 at every pixel; v = 8188.5 -> 65508: status 16;
    v = -8188.5 without ReLU: 16 (the downsample shortcut's form); with ReLU: clipped to zero before the guard, status 0.  The over-range
    launches with only the f32 NCHW output: status 0.  Every in-range output of every launch meets part B's bound."""
    print(f"\n[{binary_name()}] {route}: {ROUTE_DOC[route]}")
    for v, relu, want in [(8188.0, 1, 0), (8188.5, 1, RANGE_BIT), (-8188.5, 0, RANGE_BIT), (-8188.5, 1, 0)]:
        case = sr.conv_guard_zero_channel_case(route, v)
        planes = device_planes(case)
        ref = reference_of(case, planes, relu)
        status, hl, _ = launch_planes(case, planes, relu)
        print(f"  beta[{case['co']}] = {v}, relu = {relu}: status {status} (want {want})")
        assert status == want, (route, v, relu, status)
        ch = (hl[0].double() + hl[1].double())[..., case["co"]]
        if want == 0:
            assert bool((ch == (8.0 * v if v > 0 else 0.0)).all()) and sr.planes_well_formed(*hl)
        check_in_range_outputs("planes", planes_nchw(hl), ref, sr.PLANES_FLOOR)
        if want:       # the head's form of the same launch: no plane range, no flag, the value itself
            status, _, of32 = launch_planes(case, planes, relu, out="f32")
            print(f"  beta[{case['co']}] = {v}, relu = {relu}, f32 NCHW output only: status {status} (want 0)")
            assert status == 0 and bool((of32[:, case["co"]] == v).all())
            check_in_range_outputs("f32", of32, ref, None)


@also_on_probe_binary
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("route", list(sr.CONV_GUARD_ROUTES))
def test_conv_planes_guard_through_the_residual(route, where):
    """Random weights, inputs, BatchNorm, residual; ONE output (first pixel / first channel of the first tile, or last pixel / last valid channel
    of the last tile) is lifted by its residual to about 8300 -> status 16, or to about 8000 -> status 0 (stage_refs.conv_guard_residual_case: why
    the residual element carries 8150 / 7850 and beta the rest).  The 1 % margins are asserted on the float64 reference before the launch, so no
    f32 rounding decides.  Kernel reached: ROUTE_DOC[route]."""
    print(f"\n[{binary_name()}] {route} / {where}: {ROUTE_DOC[route]}")
    for over in (False, True):
        case = sr.conv_guard_residual_case(route, where, over)
        planes = device_planes(case)
        ref = reference_of(case, planes, 1)
        y = ref["y"].permute(0, 2, 3, 1).reshape(case["npix"], case["cout"])
        at = float(y[case["pix"], case["co"]])
        rest = y.clone()
        rest[case["pix"], case["co"]] = 0.0
        assert float(rest.abs().max()) < 0.99 * 8190.0 and (at > 1.01 * 8190.0 if over else at < 0.99 * 8190.0), (at, float(rest.abs().max()))
        status, hl, _ = launch_planes(case, planes, 1)
        print(f"  float64 output at pixel {case['pix']} / channel {case['co']} = {at:.2f}: status {status} (want {RANGE_BIT if over else 0})")
        assert status == (RANGE_BIT if over else 0)
        check_in_range_outputs("planes", planes_nchw(hl), ref, sr.PLANES_FLOOR)
        if over:
            status, _, of32 = launch_planes(case, planes, 1, out="f32")
            print(f"  f32 NCHW output only: status {status} (want 0)")
            assert status == 0
            check_in_range_outputs("f32", of32, ref, None)


@also_on_probe_binary
@pytest.mark.parametrize("route", list(sr.CONV_GUARD_ROUTES))
def test_conv_planes_guard_one_nan_input(route):
    """One NaN in a single hi-plane element of the input -> status 16, without and with ReLU (the guard's maximum propagates NaN, its comparison
    is !(<=); the ReLU in front of it must not turn the NaN into a zero that nothing reports); the outputs that do not read it are untouched."""
    case = sr.conv_guard_residual_case(route, "first", False)
    B, hw, _, cin = case["X"].shape
    k, stride = case["Wt"].shape[2], case["stride"]
    for relu in (0, 1):
        planes = device_planes(case)
        status0, clean, _ = launch_planes(case, planes, relu)
        planes[0][0][B - 1, hw // 2, hw // 2, cin - 5] = float("nan")
        status, hl, _ = launch_planes(case, planes, relu)
        got, want = planes_nchw(hl), planes_nchw(clean)
        bad = torch.isnan(got)
        print(f"[{binary_name()}] {route}, relu = {relu}: clean status {status0}, one NaN in the input hi plane: status {status} (want {RANGE_BIT}), {int(bad.sum())} NaN outputs")
        assert status0 == 0 and status == RANGE_BIT
        assert 0 < int(bad.sum()) <= case["cout"] * ((k + stride - 1) // stride) ** 2 and bool((got[~bad] == want[~bad]).all())


# ---------------------------------------------------------------------------------------------------------------- A: the stem
def _framed(x, S):
    framed = (torch.zeros(x.shape[0], S + 6, S + 8, 4, dtype=torch.float16, device=DEV), torch.zeros(x.shape[0], S + 6, S + 8, 4, dtype=torch.float16, device=DEV))
    _lib.call("gp_resize_stem_planes", _lib.ptr(x), _lib.ptr(framed[0]), _lib.ptr(framed[1]), _lib.i(x.shape[0]), _lib.i(x.shape[2]), _lib.i(x.shape[3]),
              _lib.i(S), _lib.stream_ptr())
    torch.cuda.synchronize()
    return framed


@also_on_probe_binary
def test_resize_stem_planes_guard():
    """resize_stem_planes_kernel: a 3-channel image whose float64 bilinear resize peaks at 8300 (>= 8190 x 1.01) -> status 16; at 8100
    (<= 8190 x 0.99) -> 0, and the planes hold the float64 resize to 22 bits."""
    S = 32
    for over in (False, True):
        x = sr.resize_guard_image(over)
        peak = float(sr.resize_f64(x, S).abs().max())
        assert peak >= 8190.0 * 1.01 if over else peak <= 8190.0 * 0.99
        assert _lib.take_status() == 0
        framed = _framed(x.to(DEV), S)
        status = _lib.take_status()
        print(f"[{binary_name()}] resize stem planes, float64 resize peak {peak:.1f}: status {status} (want {RANGE_BIT if over else 0})")
        assert status == (RANGE_BIT if over else 0)
        if not over:
            got = sr.planes_value(framed[0].cpu(), framed[1].cpu(), 8.0)[:, 3:S + 3, 3:S + 3, :3].permute(0, 3, 1, 2)
            assert float(got.abs().max()) == peak


@also_on_probe_binary
def test_stem_conv_planes_guard_zero_weight_channel():
    """gp_conv2d_stem_planes (conv_planes_kernel<2> with stem = 1: one kernel row per k-step, K = 224) at Cout = 128, S = 32, B = 1 (256 output
    pixels: the smallest S and B with B (S / 2)^2 % 256 = 0): the zero-weight channel cases of the other routes."""
    S, B, cout, co = 32, 1, 128, 125
    g = torch.Generator().manual_seed(12)
    framed = _framed(torch.randn(B, 3, S, S, generator=g).to(DEV), S)
    w = torch.randn(cout, 3, 7, 7, generator=g) / np.sqrt(147.0)
    w[co] = 0.0
    wplanes = planes8(sr.pack_stem_weights(w).contiguous().to(DEV), 64.0)
    ws, nb = scratch()
    xin = sr.planes_value(framed[0].cpu(), framed[1].cpu(), 8.0)
    conv = sr.stem_conv_framed_f64(xin, sr.planes_value(wplanes[0].cpu(), wplanes[1].cpu(), 64.0))
    assert _lib.take_status() == 0
    alpha = torch.ones(cout, device=DEV)
    for v, relu, want in [(8188.0, 1, 0), (8188.5, 1, RANGE_BIT), (-8188.5, 0, RANGE_BIT), (-8188.5, 1, 0)]:
        beta = torch.randn(cout, generator=torch.Generator().manual_seed(3))
        beta[co] = v
        dbeta = beta.to(DEV)
        ohi = torch.full((B * (S // 2) ** 2, cout), -7.0, dtype=torch.float16, device=DEV)
        olo = torch.full_like(ohi, -7.0)
        _lib.call("gp_conv2d_stem_planes", _lib.ptr(framed[0]), _lib.ptr(framed[1]), _lib.ptr(wplanes[0]), _lib.ptr(wplanes[1]), _lib.ptr(alpha),
                  _lib.ptr(dbeta), _lib.i(B), _lib.i(S), _lib.i(cout), _lib.i(relu), _lib.ptr(ohi), _lib.ptr(olo), _lib.ptr(ws), ctypes.c_size_t(nb),
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        status = _lib.take_status()
        print(f"[{binary_name()}] stem conv planes, beta[{co}] = {v}, relu = {relu}: status {status} (want {want})")
        assert status == want
        got = sr.planes_value(ohi.cpu(), olo.cpu(), 8.0)
        if want == 0:
            assert bool((got[:, co] == (v if v > 0 else 0.0)).all())
        ref = sr.bn_relu_f64(conv, torch.ones(cout), beta, relu).permute(0, 2, 3, 1).reshape(-1, cout)
        keep = [c for c in range(cout) if c != co]
        assert float((got[:, keep] - ref[:, keep]).abs().max()) <= 3e-6 * max(1.0, float(ref[:, keep].abs().max()))    # test_stem_conv_planes_vs_float64's bound


# ---------------------------------------------------------------------------------------------------------------- B: float64 at the ends of the range
@functools.lru_cache(maxsize=None)  # one float64 reference of a case serves both binaries
def _range_reference(name):
    case = sr.conv_range_named(name)
    wide = sr.CONV_RANGE_CASES[name][2]
    cout, k = case["cout"], case["Wt"].shape[2]
    if wide:
        from gigapose_amd.vit import split_planes

        wp = np.zeros(((cout + 127) // 128 * 128, k * k * case["X"].shape[3]), np.float32)
        wp[:cout] = case["Wt"].transpose(0, 2, 3, 1).reshape(cout, -1)
        planes = (split_planes(torch.from_numpy(case["X"]).to(DEV)), split_planes(torch.from_numpy(wp).to(DEV)), split_planes(torch.from_numpy(case["R"]).to(DEV)))
        (xh, xl), (wh, wl), (rh, rl) = planes
        x, r = sr.wide_value(xh.cpu(), xl.cpu()), sr.wide_value(rh.cpu(), rl.cpu())
        w = sr.wide_value(wh.cpu(), wl.cpu())[:cout].reshape(cout, k, k, -1).permute(0, 3, 1, 2).contiguous()
        ref = sr.conv_range_reference(x, w, case["alpha"], case["beta"], r, case["stride"], case["pad"])
    else:
        planes = device_planes(case)
        ref = reference_of(case, planes, 1)
    peak = float(ref["y"].abs().max()) / case["limit"]
    assert 0.5 <= peak <= 0.95, peak
    return case, wide, ref, peak


def launch_wide(case, planes, out="planes"):
    (xh, xl), (wh, wl), (rh, rl) = planes
    B, hw, _, cin = case["X"].shape
    cout, k, oh = case["cout"], case["Wt"].shape[2], case["oh"]
    ohi = olo = of32 = None
    if out == "planes":
        ohi = torch.full((B, oh, oh, cout), -7.0, dtype=torch.float16, device=DEV)
        olo = torch.full_like(ohi, -7.0)
    else:
        of32 = torch.full((B, cout, oh, oh), -7.0, device=DEV)
    ta, tb = torch.from_numpy(case["alpha"]).to(DEV), torch.from_numpy(case["beta"]).to(DEV)
    assert _lib.take_status() == 0
    _lib.call("gp_conv2d_nhwc_split", _lib.ptr(xh), _lib.ptr(xl), _lib.ptr(wh), _lib.ptr(wl), _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(rh), _lib.ptr(rl),
              _lib.i(B), _lib.i(hw), _lib.i(hw), _lib.i(cin), _lib.i(cout), _lib.i(k), _lib.i(k), _lib.i(case["stride"]), _lib.i(case["pad"]), _lib.i(1),
              _lib.ptr(ohi), _lib.ptr(olo), _lib.ptr(of32), _lib.stream_ptr())
    torch.cuda.synchronize()
    return _lib.take_status(), (None if ohi is None else (ohi.cpu(), olo.cpu())), (None if of32 is None else of32.cpu().double())


def wide_planes(case):
    from gigapose_amd.vit import split_planes

    cout, k = case["cout"], case["Wt"].shape[2]
    wp = np.zeros(((cout + 127) // 128 * 128, k * k * case["X"].shape[3]), np.float32)
    wp[:cout] = case["Wt"].transpose(0, 2, 3, 1).reshape(cout, -1)
    r = split_planes(torch.from_numpy(case["R"]).to(DEV)) if case["R"] is not None else (None, None)
    return split_planes(torch.from_numpy(case["X"]).to(DEV)), split_planes(torch.from_numpy(wp).to(DEV)), r


@also_on_probe_binary
@pytest.mark.parametrize("name", list(sr.CONV_RANGE_CASES))
def test_conv_vs_f64_at_the_ends_of_the_range(name):
    """stage_refs.conv_range_case: per-pixel scales 10^U(-4, 3.5) (the wide kernel: 10^U(-4, 4.4)), planted exact f16 values / rounding ties / lo
    subnormals, float64 output peaking at 0.8 of the format's limit.  Reference and bound on the values the device planes hold; EVERY output of
    both forms (planes, f32 NCHW) within c mag + floor, c = 2 x torch's own f32 error coefficient of the case, floor = the plane format's
    2^-22 |y| + its subnormal term (0 for f32).  No ordering or index decision exists here: nothing is excused."""
    case, wide, ref, peak = _range_reference(name)
    planes = wide_planes(case) if wide else device_planes(case)
    launch = launch_wide if wide else (lambda c, p, out="planes": launch_planes(c, p, 1, out))
    floor = sr.WIDE_FLOOR if wide else sr.PLANES_FLOOR
    status, hl, _ = launch(case, planes)
    status32, _, of32 = launch(case, planes, out="f32")
    got = (sr.wide_value(*hl) if wide else sr.planes_value(hl[0], hl[1], 8.0)).permute(0, 3, 1, 2)
    wp, atp = sr.conv_bound_worst(got, ref, floor)
    wf, atf = sr.conv_bound_worst(of32, ref, None)
    print(f"\n[{binary_name()}] {name} ({'gp_conv2d_nhwc_split' if wide else 'gp_conv2d_planes'}): peak |y| {peak:.3f} of the limit, c {ref['c']:.3e}, "
          f"worst err / bound planes {wp:.3f} at {atp} (y = {float(ref['y'][atp]):.4g}), f32 {wf:.3f} at {atf} (y = {float(ref['y'][atf]):.4g}); status {status} / {status32}")
    assert status == 0 and status32 == 0
    assert wp <= 1.0 and wf <= 1.0, (wp, atp, wf, atf)
    if not wide:
        assert sr.planes_well_formed(*hl)


# ---------------------------------------------------------------------------------------------------------------- D: the wide kernels at their own limit
@also_on_probe_binary
def test_wide_conv_guard_zero_weight_channel():
    """conv_split_kernel's plane epilogue: value v exactly in a zero-weight channel.  v = 65504 (the largest finite f16): status 0, hi = 65504,
    lo = 0; v = 65536 (inf in a hi plane): status 16; -65536 without ReLU: 16; the same with only the f32 NCHW output: 0, value kept."""
    case = sr.conv_guard_zero_channel_case("halo_cout64", 0.0)
    assert case["npix"] % 128 == 0
    for v, want in [(65504.0, 0), (65536.0, RANGE_BIT)]:
        case["beta"][case["co"]] = v
        planes = wide_planes(case)
        status, hl, _ = launch_wide(case, planes)
        print(f"[{binary_name()}] gp_conv2d_nhwc_split, beta[{case['co']}] = {v}: status {status} (want {want})")
        assert status == want
        if want == 0:
            assert bool((hl[0][..., case["co"]].double() == v).all()) and bool((hl[1][..., case["co"]] == 0).all())
        else:
            status, _, of32 = launch_wide(case, planes, out="f32")
            print(f"[{binary_name()}] gp_conv2d_nhwc_split, beta[{case['co']}] = {v}, f32 NCHW output only: status {status} (want 0)")
            assert status == 0 and bool((of32[:, case["co"]] == v).all())
        keep = [c for c in range(case["cout"]) if c != case["co"]]
        assert bool(torch.isfinite(hl[0][..., keep].float()).all())


@also_on_probe_binary
def test_split_weights_range_check_for_activations():
    """gp_split_weights ([C][npix] f32 -> wide planes [npix][C]: the stem's output on its way into conv_split_kernel): the host split bit for
    bit; 65504 passes, 65536 / -inf / NaN raise bit 16 (the planes written are what the conversions give: the flag reports)."""
    C, npix = 40, 300
    x = torch.randn(C, npix, generator=torch.Generator().manual_seed(4)) * 100.0
    x[3, 7] = 65504.0
    for plant, want in [(None, 0), (65536.0, RANGE_BIT), (float("-inf"), RANGE_BIT), (float("nan"), RANGE_BIT)]:
        if plant is not None:
            x[C - 1, npix - 1] = plant
        xd = x.to(DEV)
        hi, lo = torch.empty(npix, C, dtype=torch.float16, device=DEV), torch.empty(npix, C, dtype=torch.float16, device=DEV)
        assert _lib.take_status() == 0
        _lib.call("gp_split_weights", _lib.ptr(xd), _lib.i(C), _lib.i(npix), _lib.i(npix), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())
        torch.cuda.synchronize()
        status = _lib.take_status()
        print(f"[{binary_name()}] gp_split_weights, planted {plant}: status {status} (want {want})")
        assert status == want
        want_hi, want_lo = sr.split_wide_host(x.t().contiguous())
        keep = torch.ones(npix, C, dtype=torch.bool)
        if plant is not None:
            keep[npix - 1, C - 1] = False
        assert torch.equal(hi.cpu().view(torch.int16)[keep], want_hi.view(torch.int16)[keep])
        assert torch.equal(lo.cpu().view(torch.int16)[keep], want_lo.view(torch.int16)[keep])


# ---------------------------------------------------------------------------------------------------------------- C / D: the model
PLANT_FACTOR = 112.0        # the stem's BatchNorm weight x 112: chosen on the float64 forward (largest written activation 141 -> about 16000), asserted below
CROP, CROP_SCALE = 3, 112.0  # the same for ONE crop of the unplanted checkpoint
PLANE_ACT_LIMIT = 8190.0


@functools.lru_cache(maxsize=None)
def _fixture():
    from gigapose_testing import factory
    from test_gpu_e2e import make_batch

    tset = factory.TemplateSet(1, 12, seed=80)
    q = tset.crops(81, 16, "cpu")
    arrays = {n: (v.numpy() if torch.is_tensor(v) else v) for n, v in q.items()}
    return tset, q, arrays, make_batch


def _ist_f64(plant):
    """The ResNet _gigapose_with_vit builds (seed 9), in float64 on the CPU."""
    from gigapose_amd.ist_net import ISTNet, Regressor, ResNet
    from gigapose_testing import factory
    from gigapose_testing import synthetic as syn

    bb = syn.fill_state_dict(ISTNet("resnet", ResNet(dict(factory.IST_CFG)), Regressor(256, 256, True, True), 64), 9).eval().double().backbone
    if plant:
        with torch.no_grad():
            bb.bn1.weight.mul_(PLANT_FACTOR)
    return bb


@functools.lru_cache(maxsize=None)
def _planted_f64():
    """ONE float64 forward of the planted checkpoint over the 12 templates + 16 crops of the fixture (about ten seconds of CPU, shared by the
    tests below) -> (per-layer maxima, maxima of what the split path writes as planes, float64 features)."""
    tset, q, _, _ = _fixture()
    x = torch.cat([tset[0].rgb, q["tar_img"]]).double()
    return (x,) + sr.resnet_layer_maxima(_ist_f64(True), x)


def _model(plant, conv_kernel=None):
    from test_gpu_guards import _gigapose_with_vit, small_vitl

    model = _gigapose_with_vit(small_vitl(seed=11))
    bb = model.ist_net.backbone
    if plant:
        with torch.no_grad():
            bb.bn1.weight.mul_(PLANT_FACTOR)
        bb.invalidate()
    if conv_kernel is not None:
        bb.conv_kernel = conv_kernel
    model.template_datasets = {"syn": _fixture()[0]}
    return model


def _tensors(model):
    return {n: v.cpu() for n, v in model.last_predictions.tensors.items()}


def _assert_window(written, lo, hi, what):
    top = max(written.values())
    print(f"{what}: float64 maxima of what the split path writes as planes: {sr.maxima_line(written)}")
    assert lo <= top <= hi, (what, top, lo, hi)


def test_planted_checkpoint_falls_back_at_onboarding_and_equals_the_wide_model():
    """The IST twin of test_range_trip_falls_back_to_the_wide_kernels_automatically.  The stem's BatchNorm weight x 112: in the float64 torch
    forward the largest activation any layer writes lies above the planes' 8190 by 5 % and below half of the wide kernels' 65504 (asserted
    before anything is launched).  Onboarding trips bit 16 -> ResNet.conv_kernel = "128", banks rebuilt, a warning; the ViT stays on its 256
    x 256 kernels (bits 4 and 16 are independent); every tensor of last_predictions equals a model that was on "128" before onboarding, bit for
    bit; a second batch runs without another fallback."""
    _, rec, written, _ = _planted_f64()
    print(f"planted checkpoint (bn1.weight x {PLANT_FACTOR}), float64 maxima of every layer: {sr.maxima_line(rec)}")
    _assert_window(written, 1.05 * PLANE_ACT_LIMIT, 0.5 * sr.F16_MAX, "planted checkpoint")
    _, _, arrays, make_batch = _fixture()
    batch = make_batch(arrays)
    want = _model(True, "128")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want.eval_retrieval(batch, 0, "syn")
    _lib.check_status()
    ref = _tensors(want)
    model = _model(True)
    assert model.ist_net.backbone.conv_kernel == "256"
    with pytest.warns(RuntimeWarning, match="IST convolutions"):
        model.eval_retrieval(batch, 0, "syn")
    assert model.ist_net.backbone.conv_kernel == "128" and model.ae_net.dinov2_model.split_gemm == "256"
    _lib.check_status()
    got = _tensors(model)
    assert sorted(got) == sorted(ref)
    for n in ref:
        assert torch.equal(ref[n], got[n]), f"{n} differs from the model built on the wide kernels"
    for n in ("relScale", "relInplane", "pred_poses"):
        assert bool(torch.isfinite(got[n]).all()), n
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.eval_retrieval(batch, 1, "syn")
    _lib.check_status()


def test_fallen_back_backbone_on_the_planted_checkpoint_vs_float64():
    """test_ist_backbone_split_vs_chain_and_torch's bound for the wide kernels -- error <= 1.5 x the chain kernels' + 1e-7, relative to max
    |feature| -- on the planted checkpoint, where activations reach 16000 (there: below 150)."""
    x, _, _, feats = _planted_f64()
    ref = feats.numpy()
    bb = _ist_f64(True).float().to(DEV)
    xd = x.float().to(DEV)
    chain = bb.set_numerics("chain")(xd).cpu().numpy()
    bb.set_numerics("split").conv_kernel = "128"
    wide = bb(xd).cpu().numpy()
    torch.cuda.synchronize()
    _lib.check_status()
    scale = np.abs(ref).max()
    e_chain, e_wide = (np.abs(v - ref).max() / scale for v in (chain, wide))
    print(f"IST backbone, planted checkpoint (max |feature| {scale:.4g}), vs float64 torch over 28 images: chain {e_chain:.2e}, split-128 {e_wide:.2e}")
    assert e_wide <= 1.5 * e_chain + 1e-7


def _scaled_crop_maxima(scale):
    _, q, _, _ = _fixture()
    return sr.resnet_layer_maxima(_ist_f64(False), q["tar_img"][CROP:CROP + 1].double() * scale)[1]


def _with_scaled_crop(scale):
    _, _, arrays, make_batch = _fixture()
    big = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in arrays.items()}
    big["tar_img"][CROP] *= scale
    return make_batch(big)


def test_one_large_crop_trips_the_fallback_after_a_clean_onboarding():
    """The unplanted checkpoint onboards cleanly; then crop 3 x 112 (float64: over the planes' limit by 5 %, inside half of the wide range) ->
    the fallback warning, a clean status word, finite relScale / relInplane / pred_poses for all 16 crops, and the 15 untouched crops equal
    a model on "128" from the start bit for bit."""
    _assert_window(_scaled_crop_maxima(CROP_SCALE), 1.05 * PLANE_ACT_LIMIT, 0.5 * sr.F16_MAX, f"crop {CROP} x {CROP_SCALE}")
    batch = _with_scaled_crop(CROP_SCALE)
    want = _model(False, "128")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want.eval_retrieval(batch, 0, "syn")
    _lib.check_status()
    ref = _tensors(want)
    model = _model(False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.set_template_data("syn")
    _lib.check_status()
    assert model.ist_net.backbone.conv_kernel == "256"
    with pytest.warns(RuntimeWarning, match="IST convolutions"):
        model.eval_retrieval(batch, 0, "syn")
    assert model.ist_net.backbone.conv_kernel == "128"
    _lib.check_status()
    got = _tensors(model)
    keep = [i for i in range(16) if i != CROP]
    for n in ("relScale", "relInplane", "pred_poses"):
        assert bool(torch.isfinite(got[n]).all()), n
        assert torch.equal(got[n][keep], ref[n][keep]), f"{n} of an untouched crop differs from the model built on the wide kernels"


def _flow(model, tmp, images):
    import os

    log_dir = str(tmp)
    os.makedirs(os.path.join(log_dir, "predictions"), exist_ok=True)
    model.log_dir, model.test_dataset_name, model.run_id, model.accumulate_crops = log_dir, "syn", "r0", 64
    for i, b in enumerate(images):
        assert model.test_step(b, i) == 0
    model.flush_pending()
    torch.cuda.synchronize()
    _lib.check_status()
    out = []
    for i in range(len(images)):
        with np.load(os.path.join(log_dir, "predictions", f"{i}.npz")) as z:
            out.append({k: z[k] for k in z.files})
    return out


def _two_images(scale=None):
    _, _, arrays, make_batch = _fixture()
    images = []
    for part in (slice(0, 8), slice(8, 16)):
        a = {n: (v[part].copy() if isinstance(v, np.ndarray) else v[part]) for n, v in arrays.items()}
        if scale is not None and part.start <= CROP < part.stop:
            a["tar_img"][CROP - part.start] *= scale
        images.append(make_batch(a))
    return images


@pytest.mark.parametrize("trip", ["planted_checkpoint", "large_crop"])
def test_accumulated_flow_falls_back_once_and_writes_the_wide_models_files(trip, tmp_path):
    """test_step through the queue (accumulate_crops = 64): two images of 8 crops, one flush at the end.  planted_checkpoint: the flush onboards,
    onboarding trips and widens.  large_crop (unplanted checkpoint, crop 3 x 112): the bank onboards cleanly and the FLUSH trips -- the retry
    loop of _finish_flush.  Either way exactly one fallback warning, and the files equal those of a model on "128" from the start (`time` aside)."""
    plant = trip == "planted_checkpoint"
    scale = None if plant else CROP_SCALE
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want = _flow(_model(plant, "128"), tmp_path / "want", _two_images(scale))
    model = _model(plant)
    if not plant:
        model.set_template_data("syn")
        _lib.check_status()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = _flow(model, tmp_path / "got", _two_images(scale))
    falls = [w for w in caught if issubclass(w.category, RuntimeWarning) and "IST convolutions" in str(w.message)]
    assert len(falls) == 1, [str(w.message) for w in caught]
    assert model.ist_net.backbone.conv_kernel == "128" and model.ae_net.dinov2_model.split_gemm == "256"
    for a, b in zip(want, got):
        assert sorted(a) == sorted(b)
        for key in a:
            if key != "time":
                assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
        assert np.isfinite(b["poses"]).all() and np.isfinite(b["scores"]).all()


def test_beyond_the_wide_range_raises_instead_of_returning_garbage():
    """After the fallback (conv_kernel "128") a crop whose float64 per-layer maximum exceeds 65504 by more than 5 % (crop 3 x 1e5: the stem's
    output alone is over a million) must raise GigaPoseHipError with bit 16's message -- from gp_split_weights / conv_split_kernel's plane
    epilogue -- and never return relScale / relInplane / pred_poses under a clean status word.  The model is usable afterwards."""
    written = _scaled_crop_maxima(1.0e5)
    print(f"crop {CROP} x 1e5, float64 maxima of what the split path writes as planes: {sr.maxima_line(written)}")
    assert max(written.values()) > 1.05 * sr.F16_MAX
    _, _, arrays, make_batch = _fixture()
    model = _model(False, "128")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.eval_retrieval(make_batch(arrays), 0, "syn")
    _lib.check_status()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # the ViT sees the crop as well and may re-calibrate its plane scales on the way (bit 4): not this test's business
        with pytest.raises(_lib.GigaPoseHipError, match="IST activation left the range"):
            model.eval_retrieval(_with_scaled_crop(1.0e5), 1, "syn")
    assert _lib.take_status() == 0                        # reading cleared it
    assert model.ist_net.backbone.conv_kernel == "128"
    model.eval_retrieval(make_batch(arrays), 2, "syn")    # the model is usable afterwards
    _lib.check_status()
    for n in ("relScale", "relInplane", "pred_poses"):
        assert bool(torch.isfinite(model.last_predictions.tensors[n]).all()), n


@pytest.mark.parametrize("scale,legal", [(CROP_SCALE, True), (2.0e3, False), (1.0e5, False)])
def test_wide_resnet_forward_never_returns_non_finite_features_silently(scale, legal):
    """ResNet.forward with conv_kernel "128" on crop 3 x scale.  x 112: inside the wide range by float64 -> finite, status 0.  x 2000: the f32
    stem's output is legal (float64: below 65504) and a later layer is not -> conv_split_kernel's plane epilogue must flag it.  x 1e5: the stem's
    output itself -> gp_split_weights must.  Non-finite features under a clean status word are the failure this test exists for."""
    written = _scaled_crop_maxima(scale)
    top = max(written.values())
    print(f"crop {CROP} x {scale}: float64 stem output {written['relu(bn1)']:.4g}, largest written activation {top:.4g}")
    if legal:
        assert top < 0.5 * sr.F16_MAX
    else:
        assert top > 1.05 * sr.F16_MAX and (written["relu(bn1)"] < 0.95 * sr.F16_MAX) == (scale < 1.0e4)
    _, q, _, _ = _fixture()
    bb = _ist_f64(False).float().to(DEV).set_numerics("split")
    bb.conv_kernel = "128"
    x = q["tar_img"][:4].clone()
    x[CROP] *= scale
    feats = bb(x.to(DEV))
    torch.cuda.synchronize()
    status = _lib.take_status()
    finite = bool(torch.isfinite(feats).all())
    print(f"  features finite: {finite}, status {status}")
    assert status == (0 if legal else RANGE_BIT)
    assert finite or status & RANGE_BIT
    assert bool(torch.isfinite(feats[:CROP]).all())        # the other crops of the batch are untouched
