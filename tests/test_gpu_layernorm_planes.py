"""GPU: LayerNorm -> activation planes (gp_layernorm_planes; gp_vit.hip: launch_layernorm_planes) against float64, branch by branch.

The plane path runs this launch twice per ViT layer; until now only whole ViT forwards reached it.  Every dispatch branch is driven
through the C-ABI on its own -- layernorm_planes_reg_kernel<8, 16>, <8, 32>, <6, 32> and the three-pass layernorm_planes_kernel -- on
channel-major inputs whose token classes (gigapose_testing/stage_refs.py: layernorm_case) are what kernels of this kind get wrong:
DINOv2-like massive channels, a common offset far above the spread, zero variance, pad columns; each class at the first and last
column of a block, in its middle and at the end of the buffer.  Asserted per case:
  * against float64 per token class, e = |(hi + lo) / 8 - y64| / (|gamma| (|xhat| + 1) + |beta|), bounded by the error of ATen's f32
    LayerNorm on the CPU on the same inputs (same measure, same class) and of a numpy f32 model of the branch's own summation order,
    see LN_MARGIN / LN_MODEL_MARGIN;
  * constant and pad tokens: planes == split(8 beta) bit for bit;  planes well formed everywhere (|lo| <= ulp(hi) / 2, finite);
  * permuting the token columns permutes the plane rows and changes no bit (catches a transpose / LDS-index slip without a tolerance);
  * the branches agree to the sum of their bounds;  the status word stays 0;  a value beyond the planes' range raises the range bit.
Which branch a case takes follows from the conditions in launch_layernorm_planes (restated per case below), not from timing."""
import ctypes

import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
F = torch.nn.functional

# The kernel may have at most LN_MARGIN x the class's maximum of the f32 CPU reference + 2^-22 (the planes' 22 bits).  The factor covers a
# different summation order (16 or 32 sequential partial sums per token instead of ATen's) on a single-sample maximum; nothing else.
# That margin was set without a GPU measurement and is too small for the `offset` class (mean 50, spread 0.6 .. 3: the error is the
# round-off of the mean, and ATen's vectorised tree sum carries less of it than 16 / 32 sequential sums of 64 / 32 values near 50 each).
# Measured on an MI355X (profiles/stage_tests_vs_float64.txt): reg<8,16> offset 1.349e-5 and reg<8,32> at Mpad = 2304 1.180e-5 against
# 2 x 5.49e-6 + 2^-22 = 1.12e-5 -- and the numpy f32 model of exactly these summation orders (stage_refs.layernorm_partial_sums_f32: the
# same partial sums in the same order on the CPU) gives 1.349e-5 and 1.180e-5 against float64, the same excess to three digits.  So the
# arithmetic is what it is documented to be and the margin was too small: a class's bound is the larger of LN_MARGIN x the ATen figure and
# LN_MODEL_MARGIN x the model's figure for the branch's order, + 2^-22.  Every other class stays inside the factor 2 on its own.
LN_MARGIN = 2.0
LN_MODEL_MARGIN = 1.25


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def ln_planes(x_tm, gamma, beta):
    """x_tm [Mpad][C] f32 on the CPU (token-major) -> planes (hi, lo) [Mpad][C] on the CPU; the kernel reads X [C][Mpad]."""
    Mpad, C = x_tm.shape
    X = x_tm.to(DEV).t().contiguous()
    hi = torch.zeros(Mpad, C, dtype=torch.float16, device=DEV)
    lo = torch.zeros_like(hi)
    g, b = gamma.to(DEV), beta.to(DEV)
    _lib.call("gp_layernorm_planes", _lib.ptr(X), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(g), _lib.ptr(b), _lib.i(C), _lib.i(Mpad), _lib.f(EPS),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return hi.cpu(), lo.cpu()


def bits(t):
    return t.view(torch.int16)


def reference_bounds(x, cls, gamma, beta, slices, contiguous):
    """float64 LayerNorm, and per class the error of the two references the bound is taken from: ATen's f32 LayerNorm on the CPU, and the
    numpy f32 model of the branch's summation order (`slices` partial sums per token, interleaved or contiguous)."""
    y, xhat = sr.layernorm_f64(x, gamma, beta, EPS)
    ref = sr.per_class_max(sr.layernorm_error(F.layer_norm(x, (x.shape[1],), gamma, beta, EPS), y, xhat, gamma, beta), cls)
    model = sr.per_class_max(sr.layernorm_error(torch.from_numpy(sr.layernorm_partial_sums_f32(x.numpy(), gamma.numpy(), beta.numpy(), EPS, slices,
                                                                                                  contiguous)), y, xhat, gamma, beta), cls)
    bound = {k: max(LN_MARGIN * ref[k], LN_MODEL_MARGIN * model[k]) + sr.PLANE_BITS for k in ref}
    return y, xhat, ref, model, bound


def check_case(tag, C, Mpad, seed, slices, contiguous):
    """One branch on one input: every assertion of the module docstring except the cross-branch one.  `slices`, `contiguous`: the
    summation order of the branch, for the numpy f32 model the bound takes into account.  Returns what the cross-branch test needs."""
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, seed)
    hi, lo = ln_planes(x, gamma, beta)
    _lib.check_status()
    y, xhat, ref, model, bound = reference_bounds(x, cls, gamma, beta, slices, contiguous)
    got = sr.per_class_max(sr.layernorm_error(sr.planes_value(hi, lo, 8.0), y, xhat, gamma, beta), cls)
    for k in got:
        print(f"LN planes {tag} C={C} Mpad={Mpad} class {k:8s}: kernel {got[k]:.3e}  f32 CPU reference {ref[k]:.3e}  ratio "
              f"{got[k] / ref[k] if ref[k] else float('nan'):.2f}  bound {bound[k]:.3e}  (numpy f32 model of the branch's summation order {model[k]:.3e})")
    assert sr.planes_well_formed(hi, lo), tag
    # constant and pad tokens: x - mean is exactly 0 in any summation order -> planes of 8 beta, bit for bit
    flat = (cls == 3) | (cls == 4)
    bh, bl = sr.split_planes_host(beta, 8.0)
    assert int(flat.sum()) >= 10
    assert torch.equal(bits(hi[flat]), bits(bh.expand(int(flat.sum()), C))) and torch.equal(bits(lo[flat]), bits(bl.expand(int(flat.sum()), C))), tag
    for k in got:
        assert got[k] <= bound[k], (tag, k, got[k], ref[k], bound[k])
    # position independence: the arithmetic of a token does not depend on its lane, block or neighbours
    perm = torch.from_numpy(np.random.RandomState(seed + 1).permutation(Mpad))
    phi, plo = ln_planes(x[perm], gamma, beta)
    _lib.check_status()
    assert torch.equal(bits(phi), bits(hi[perm])) and torch.equal(bits(plo), bits(lo[perm])), f"{tag}: a token's planes depend on its column"
    return x, cls, gamma, beta, hi, lo, bound


# natural dispatch (product library), launch_layernorm_planes:
#   C == 1024 && Mpad % 32 == 0 && Mpad / 32 <= 128  -> layernorm_planes_reg_kernel<8, 16>  (2304 / 32 = 72 blocks of 32: the 16-token form)
#   C == 1024 && Mpad % 32 == 0                      -> layernorm_planes_reg_kernel<8, 32>  (16640 / 32 = 520 > 128)
#   C == 768 && Mpad % 32 == 0                       -> layernorm_planes_reg_kernel<6, 32>
#   any other width                                  -> layernorm_planes_kernel (three passes, 64-token blocks, 16 contiguous slices)
NATURAL = [("reg<8,16>", 1024, 2304, 16 * 2, False),       # TOK = 16: 512 / 16 = 32 slices
           ("reg<8,32>", 1024, 16640, 16, False),          # TOK = 32: 16 slices
           ("reg<6,32>", 768, 2304, 16, False),
           ("three-pass-384", 384, 2304, 16, True),
           ("three-pass-1280", 1280, 2304, 16, True)]


@pytest.mark.parametrize("tag,C,Mpad,slices,contiguous", NATURAL, ids=[c[0] for c in NATURAL])
def test_layernorm_planes_branch_vs_float64(tag, C, Mpad, slices, contiguous):
    check_case(tag, C, Mpad, 100 + C + Mpad, slices, contiguous)


def set_ln_reg(mode):
    _lib.lib().gp_vit_set_ln_reg(ctypes.c_int(mode))


# the probe hook (probe library), same function: g_ln_planes_reg == 0 skips the three register branches -> layernorm_planes_kernel at
# C = 1024; == 2 fails the first condition (`!= 2`) and takes the second -> layernorm_planes_reg_kernel<8, 32> at Mpad = 2304
HOOKED = [("three-pass-1024 (ln_reg 0)", 0, 16, True), ("reg<8,32> at 72 blocks (ln_reg 2)", 2, 16, False)]


@pytest.mark.probes
@pytest.mark.parametrize("tag,mode,slices,contiguous", HOOKED, ids=["ln_reg0", "ln_reg2"])
def test_layernorm_planes_hooked_branch_vs_float64(tag, mode, slices, contiguous):
    try:
        set_ln_reg(mode)
        check_case(tag, 1024, 2304, 100 + 1024 + 2304, slices, contiguous)
    finally:
        set_ln_reg(1)


@pytest.mark.probes
def test_layernorm_planes_branches_agree():
    """C = 1024, Mpad = 2304 through the 16-token form (hook 1), the three-pass kernel (hook 0) and the 32-token form (hook 2): documented
    as agreeing "to f32 round-off, not bit for bit" -- here: to the sum of the two branches' bounds against float64, per class; the
    constant / pad tokens (no round-off at all) bit for bit."""
    C, Mpad = 1024, 2304
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, 100 + C + Mpad)
    order = {1: (32, False), 0: (16, True), 2: (16, False)}              # hook -> (partial sums per token, contiguous slices)
    bound = {}
    for mode, (slices, contiguous) in order.items():
        y, xhat, _, _, bound[mode] = reference_bounds(x, cls, gamma, beta, slices, contiguous)
    out = {}
    try:
        for mode in (1, 0, 2):
            set_ln_reg(mode)
            out[mode] = ln_planes(x, gamma, beta)
            _lib.check_status()
    finally:
        set_ln_reg(1)
    den = gamma.double().abs() * (xhat.abs() + 1.0) + beta.double().abs()
    for a, b in ((1, 0), (1, 2), (0, 2)):
        d = (sr.planes_value(*out[a], 8.0) - sr.planes_value(*out[b], 8.0)).abs() / den
        dm = sr.per_class_max(d, cls)
        print(f"LN planes ln_reg {a} vs {b}: " + ", ".join(f"{k} {v:.2e} (<= {bound[a][k] + bound[b][k]:.2e})" for k, v in dm.items()))
        for k, v in dm.items():
            assert v <= bound[a][k] + bound[b][k], (a, b, k, v)
        flat = (cls == 3) | (cls == 4)
        assert torch.equal(bits(out[a][0][flat]), bits(out[b][0][flat])) and torch.equal(bits(out[a][1][flat]), bits(out[b][1][flat]))
    assert not torch.equal(bits(out[1][1]), bits(out[0][1])), "hook 0 and hook 1 produced identical lo planes: the hook did not switch the kernel"


@pytest.mark.parametrize("C,Mpad", [(1024, 2304), (768, 2304), (384, 2304)])
def test_layernorm_planes_range_guard(C, Mpad):
    """One gamma scaled so that |8 y| > 65504 on the massive channel (xhat there is 15 .. 25): GP_STATUS_SPLIT_RANGE, a status bit -- and
    without it the word stays clean on the same input."""
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, 7)
    ln_planes(x, gamma, beta)
    _lib.check_status()
    _, xhat = sr.layernorm_f64(x, gamma, beta, EPS)
    g2 = gamma.clone()
    g2[sr.LN_MASSIVE[0][0]] = 1.2 * 8190.0 / float(xhat[cls == 1][:, sr.LN_MASSIVE[0][0]].abs().min())
    ln_planes(x, g2, beta)
    with pytest.raises(_lib.GigaPoseHipError, match="range of the f16 planes"):
        _lib.check_status()
    assert _lib.take_status() == 0


def test_layernorm_planes_argument_errors():
    x = torch.zeros(1024, 128, device=DEV)
    hi = torch.zeros(128, 1024, dtype=torch.float16, device=DEV)
    lo = torch.zeros_like(hi)
    g = torch.ones(1024, device=DEV)

    def call(X, h, l, ga, be, C, Mpad):
        _lib.call("gp_layernorm_planes", _lib.ptr(X), _lib.ptr(h), _lib.ptr(l), _lib.ptr(ga), _lib.ptr(be), _lib.i(C), _lib.i(Mpad), _lib.f(EPS),
                  _lib.stream_ptr())

    call(x, hi, lo, g, g, 1024, 128)
    for bad in (dict(C=100), dict(Mpad=96), dict(X=None), dict(h=None), dict(l=None), dict(ga=None), dict(be=None)):
        kw = dict(X=x, h=hi, l=lo, ga=g, be=g, C=1024, Mpad=128)
        kw.update(bad)
        with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_layernorm_planes"):
            call(**kw)
    torch.cuda.synchronize()
    _lib.check_status()
