"""GPU: the ResNet stem in split numerics, stage by stage -- gp_resize_stem_planes (bilinear resize into zero-framed 4-channel planes)
and gp_conv2d_stem_planes (conv_planes_kernel with a.stem = 1: one kernel row of 8 taps x 4 channels per k-step, K = 224).

Until now only the whole ResNet at B = 3, 224 -> 256, Cout = 128 reached them.  Here: Cout = 192 / 256 (three / four matrix column blocks
with the one-kernel-row k-step), B = 1 / 2 (64 / 128 tiles of 7 k-steps on a 256-slot launch: fewer than two k-steps per slot, the
shortest k-ranges the hand-over scheme sees), B = 4 (one tile per slot), B = 5 (a remainder), non-square inputs, the zero frame and the
zero 4th channel, and scratch reuse across launches (epoch-tagged hand-overs).  The float64 reference of the convolution is evaluated
on the values the planes actually hold, in the framed layout (gigapose_testing/stage_refs.py: stem_conv_framed_f64, pinned to
F.conv2d(stride 2, padding 3) in tests/test_stage_refs.py), so that only the kernel's arithmetic is measured."""
import ctypes

import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from gigapose_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = torch.nn.functional


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def bits(t):
    return t.cpu().view(torch.int16)


def resize(images, S, framed):
    B, _, IH, IW = images.shape
    _lib.call("gp_resize_stem_planes", _lib.ptr(images), _lib.ptr(framed[0]), _lib.ptr(framed[1]), _lib.i(B), _lib.i(IH), _lib.i(IW), _lib.i(S),
              _lib.stream_ptr())
    torch.cuda.synchronize()


def new_frame(B, S):
    return (torch.zeros(B, S + 6, S + 8, 4, dtype=torch.float16, device=DEV), torch.zeros(B, S + 6, S + 8, 4, dtype=torch.float16, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("IH,IW,S", [(224, 224, 256), (200, 312, 256), (256, 256, 256), (224, 224, 32), (37, 53, 64)])
def test_resize_stem_planes_vs_float64(IH, IW, S):
    """Two different inputs in a row into buffers zeroed once.  Interior against float64 bilinear / align_corners: at most 2 x the maximum
    error of the same call in f32 on the CPU (measured here) + 2^-22 relative for the planes (+ their subnormal floor) -- the factor is for the contraction order
    of the four products only; frame and 4th channel all zero after both calls; IH = IW = S: the planes of 8 x, bit for bit."""
    B = 3
    framed = new_frame(B, S)
    g = torch.Generator().manual_seed(IH * 1000 + IW + S)
    for call in range(2):
        x = torch.randn(B, 3, IH, IW, generator=g) * (1.0 + call)
        resize(x.to(DEV), S, framed)
        _lib.check_status()
        hi, lo = framed[0].cpu(), framed[1].cpu()
        r64 = sr.resize_f64(x, S)
        r32 = F.interpolate(x, (S, S), mode="bilinear", align_corners=True)
        e_ref = float((r32.double() - r64).abs().max())
        inner = sr.planes_value(hi, lo, 8.0)[:, 3:S + 3, 3:S + 3, :3].permute(0, 3, 1, 2)
        err = (inner - r64).abs()
        # the planes: 22 bits of 8 x down to the f16 subnormal floor of the lo plane (2^-25 of 8 x, absolute)
        bound = 2.0 * e_ref + sr.PLANE_BITS * r64.abs() + 2.0 ** -25 / 8.0
        print(f"resize stem planes {IH}x{IW} -> {S}, call {call}: kernel max err {float(err.max()):.3e}, f32 CPU reference {e_ref:.3e}, "
              f"ratio {float(err.max()) / e_ref if e_ref else float('nan'):.2f}, worst err - bound {float((err - bound).max()):.2e}")
        assert bool((err <= bound).all())
        assert sr.planes_well_formed(hi, lo)
        if IH == S and IW == S:      # interpolation weights exactly 1 and 0
            want_hi, want_lo = sr.split_planes_host(x.permute(0, 2, 3, 1).contiguous(), 8.0)
            assert torch.equal(bits(hi[:, 3:S + 3, 3:S + 3, :3].contiguous()), bits(want_hi))
            assert torch.equal(bits(lo[:, 3:S + 3, 3:S + 3, :3].contiguous()), bits(want_lo))
        for p in (hi, lo):           # 3 rows / columns before, 3 rows / 5 columns after, channel 3: zero words (+0)
            w = p.view(torch.int16)
            assert bool((w[:, :3] == 0).all()) and bool((w[:, S + 3:] == 0).all()) and bool((w[:, :, :3] == 0).all())
            assert bool((w[:, :, S + 3:] == 0).all()) and bool((w[..., 3] == 0).all())


def test_resize_stem_planes_argument_errors():
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    framed = new_frame(1, 32)
    resize(x, 32, framed)
    with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_resize_stem_planes"):
        resize(x, 31, framed)
    for ptrs in ((None, framed[0], framed[1]), (x, None, framed[1]), (x, framed[0], None)):
        with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_resize_stem_planes"):
            _lib.call("gp_resize_stem_planes", _lib.ptr(ptrs[0]), _lib.ptr(ptrs[1]), _lib.ptr(ptrs[2]), _lib.i(1), _lib.i(16), _lib.i(16), _lib.i(32),
                      _lib.stream_ptr())
    torch.cuda.synchronize()
    _lib.check_status()


# ---------------------------------------------------------------------------------------------------------------- convolution
def stem_module(cout, seed):
    """A ResNet whose stem has `cout` channels: the weight planes come from ResNet._pack_planes (the product's packing, not restated)."""
    from gigapose_amd.ist_net import ResNet
    from test_oracle_pose_ist import IST_CFG

    torch.manual_seed(seed)
    net = ResNet(dict(IST_CFG, initial_dim=cout)).eval()
    with torch.no_grad():
        net.conv1.weight.copy_(torch.randn(cout, 3, 7, 7, generator=torch.Generator().manual_seed(seed)) / np.sqrt(147.0))
    net = net.to(DEV)
    net._pack_planes(torch.device(DEV, torch.cuda.current_device()))
    return net


def scratch():
    lib = _lib.lib()
    nb = lib.gp_conv2d_planes_workspace_bytes()
    return torch.zeros((nb + 3) // 4, dtype=torch.float32, device=DEV), nb


def stem_conv(framed, wplanes, alpha, beta, B, S, cout, relu, ws, nb):
    npix = B * (S // 2) * (S // 2)
    ohi = torch.full((npix, cout), -7.0, dtype=torch.float16, device=DEV)
    olo = torch.full((npix, cout), -7.0, dtype=torch.float16, device=DEV)
    _lib.call("gp_conv2d_stem_planes", _lib.ptr(framed[0]), _lib.ptr(framed[1]), _lib.ptr(wplanes[0]), _lib.ptr(wplanes[1]), _lib.ptr(alpha),
              _lib.ptr(beta), _lib.i(B), _lib.i(S), _lib.i(cout), _lib.i(relu), _lib.ptr(ohi), _lib.ptr(olo), _lib.ptr(ws), ctypes.c_size_t(nb),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return ohi, olo


def framed_input(B, seed, S=256):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 224, 224, generator=g) * (0.5 + 2.0 * torch.rand(B, 1, 1, 1, generator=g))
    framed = new_frame(B, S)
    resize(x.to(DEV), S, framed)
    return framed


STEM_CASES = [(128, 1, True, 1), (128, 2, True, 1), (128, 3, True, 1), (128, 4, True, 1), (128, 5, True, 1),
              (192, 1, True, 1), (192, 4, True, 1), (256, 1, True, 1), (256, 4, True, 1),
              (128, 2, False, 1),       # alpha = beta = NULL
              (192, 1, True, 0)]        # no ReLU


@pytest.mark.parametrize("cout,B,bn,relu", STEM_CASES, ids=[f"co{c}-B{b}{'' if bn else '-nobn'}{'' if r else '-norelu'}" for c, b, bn, r in STEM_CASES])
def test_stem_conv_planes_vs_float64(cout, B, bn, relu):
    """S = 256 (128 x 128 outputs: 64 B tiles of 256 pixels x 7 k-steps on 256 slots).  Against float64 conv + BN + ReLU on the plane
    values, tolerance = the project's figure for conv_planes_kernel's plane output (test_conv_planes_vs_f64): 3e-6 max(1, max |y|).
    A second launch on the same scratch gives the same bits."""
    S = 256
    net = stem_module(cout, 40 + cout)
    wplanes = net._planes["stem"]
    assert wplanes is not None and wplanes[0].shape == (cout, 224)
    framed = framed_input(B, 500 + cout + B)
    rs = np.random.RandomState(cout + B)
    alpha = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32)) if bn else None
    beta = torch.from_numpy(rs.standard_normal(cout).astype(np.float32)) if bn else None
    ws, nb = scratch()
    da, db = (alpha.to(DEV), beta.to(DEV)) if bn else (None, None)
    ohi, olo = stem_conv(framed, wplanes, da, db, B, S, cout, relu, ws, nb)
    _lib.check_status()
    ohi2, olo2 = stem_conv(framed, wplanes, da, db, B, S, cout, relu, ws, nb)
    _lib.check_status()
    assert torch.equal(bits(ohi), bits(ohi2)) and torch.equal(bits(olo), bits(olo2)), "two launches on one scratch differ"
    xin = sr.planes_value(framed[0].cpu(), framed[1].cpu(), 8.0)
    wk = sr.planes_value(wplanes[0].cpu(), wplanes[1].cpu(), 64.0)
    ref = sr.bn_relu_f64(sr.stem_conv_framed_f64(xin, wk), alpha, beta, relu)                       # (B, cout, 128, 128)
    got = sr.planes_value(ohi.cpu(), olo.cpu(), 8.0).reshape(B, S // 2, S // 2, cout).permute(0, 3, 1, 2)
    tol = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"stem conv planes Cout={cout} B={B} bn={bn} relu={relu}: max err / max(1, max|y|) = {err / tol:.3e} (max |y| {float(ref.abs().max()):.2f}; bound 3e-6)")
    assert sr.planes_well_formed(ohi.cpu(), olo.cpu())
    assert err <= 3e-6 * tol, (err, tol)
    if not relu:
        assert float(ref.min()) < -0.5 and float(got.min()) < -0.5       # negative outputs survive


def test_stem_conv_scratch_reuse_across_shapes():
    """One scratch, launches of different shapes in a row (B = 1 / Cout = 192: cut tiles; B = 5 / Cout = 128: a remainder; B = 2 / Cout =
    256): every launch equals the same launch on a freshly zeroed scratch, bit for bit (hand-overs are tagged with a per-launch epoch)."""
    S = 256
    ws, nb = scratch()
    shapes = [(192, 1), (128, 5), (256, 2), (192, 1), (128, 2), (128, 5)]
    mods = {c: stem_module(c, 40 + c) for c in (128, 192, 256)}
    ins = {b: framed_input(b, 900 + b) for b in (1, 2, 5)}
    fresh = {}
    for cout, B in shapes:
        a = torch.linspace(0.5, 1.5, cout, device=DEV)
        b = torch.linspace(-1.0, 1.0, cout, device=DEV)
        if (cout, B) not in fresh:
            w0, _ = scratch()
            fresh[(cout, B)] = stem_conv(ins[B], mods[cout]._planes["stem"], a, b, B, S, cout, 1, w0, nb)
        ohi, olo = stem_conv(ins[B], mods[cout]._planes["stem"], a, b, B, S, cout, 1, ws, nb)
        assert torch.equal(bits(ohi), bits(fresh[(cout, B)][0])) and torch.equal(bits(olo), bits(fresh[(cout, B)][1])), (cout, B)
        assert not bool((bits(ohi) == bits(torch.tensor([-7.0], dtype=torch.float16))).all(dim=1).any()), "an output row was not written"
    _lib.check_status()


def test_stem_conv_argument_errors():
    """Refused before anything is launched: Cout = 64, a pixel count that is not a multiple of 256, alpha without beta, a NULL plane."""
    net = stem_module(128, 168)
    framed = new_frame(1, 32)
    ws, nb = scratch()
    a = torch.ones(128, device=DEV)
    with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_conv2d_stem_planes"):
        stem_conv(framed, net._planes["stem"], a, a, 1, 32, 64, 1, ws, nb)             # Cout = 64
    f24 = new_frame(1, 24)
    with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_conv2d_stem_planes.*multiple of 256"):
        stem_conv(f24, net._planes["stem"], a, a, 1, 24, 128, 1, ws, nb)               # 144 pixels
    with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_conv2d_stem_planes"):
        stem_conv(framed, net._planes["stem"], a, None, 1, 32, 128, 1, ws, nb)         # alpha without beta
    with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_conv2d_stem_planes"):
        stem_conv((None, framed[1]), net._planes["stem"], a, a, 1, 32, 128, 1, ws, nb)
    _lib.check_status()


# ---------------------------------------------------------------------------------------------------------------- host mirror
def _ist_backbone():
    from test_oracle_pose_ist import build_ist

    return build_ist(101)


@pytest.mark.parametrize("B", [1, 5])
def test_resnet_split_other_batch_sizes_vs_chain_and_torch(B):
    """ResNet.forward in split numerics at B = 1 and B = 5 within the bound test_ist_backbone_split_vs_chain_and_torch sets at B = 3:
    2e-5 of max |feature| against the float64 torch forward, and <= 1.5 x the chain mode + 1e-7."""
    from oracle import ist_torch

    net = _ist_backbone()
    tmpl, _ = syn.template_images(102, 2)
    pool = np.concatenate([tmpl, tmpl[:1] * 0.5, tmpl[::-1] * 0.8])
    x = torch.from_numpy(np.ascontiguousarray(pool[:B]))
    with torch.no_grad():
        ref = ist_torch.resnet_forward(net.backbone.double(), x.double()).numpy()
    net = net.float().to(DEV)
    chain = net.backbone.set_numerics("chain")(x.to(DEV)).cpu().numpy()
    split = net.backbone.set_numerics("split")(x.to(DEV)).cpu().numpy()
    torch.cuda.synchronize()
    _lib.check_status()
    scale = np.abs(ref).max()
    e_chain, e_split = (np.abs(v - ref).max() / scale for v in (chain, split))
    print(f"IST backbone B={B} vs f64 torch: chain {e_chain:.2e}, split {e_split:.2e} (relative to max |feature|)")
    assert e_split < 2e-5 and e_split <= 1.5 * e_chain + 1e-7


def test_resnet_split_batch_size_sequence_equals_fresh_modules():
    """B = 3, 5, 3 on ONE module (_framed and _stem_planes are re-allocated by batch size, the scratch is kept) == fresh modules, bit for bit."""
    tmpl, _ = syn.template_images(102, 2)
    pool = torch.from_numpy(np.ascontiguousarray(np.concatenate([tmpl, tmpl[:1] * 0.5, tmpl[::-1] * 0.8]))).to(DEV)
    one = _ist_backbone().float().to(DEV).backbone.set_numerics("split")
    for B in (3, 5, 3):
        got = one(pool[:B]).clone()
        fresh = _ist_backbone().float().to(DEV).backbone.set_numerics("split")(pool[:B])
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), fresh.view(torch.int32)), B
    _lib.check_status()
