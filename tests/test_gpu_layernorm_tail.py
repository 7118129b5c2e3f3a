"""GPU: the tail of a LayerNorm -> planes launch (gp_vit.hip: launch_layernorm_planes, layernorm_planes_reg_kernel<NK, 32, FOLD>).

With the live-token count of the forward (B * 257 of Mpad rows; here set through the probe library's gp_vit_set_ln_live), blocks of
pure row padding do not run -- their plane rows are zeroed -- and when the 32-token blocks exceed a whole number of resident rounds
by at most 4, the remainder's tokens ride as extra tokens on first-round blocks (at ViT-L x 64 crops: 514 blocks on 512 slots).
An extra token is summed in a regular token's order, so its planes must not depend on where it sits.

Shapes: the smallest that reach each path, from the device's CU count (two 512-thread blocks are resident per CU: S slots) --
remainder 1 block, 2 blocks, 2 with the last one partial, none -- with and without blocks of pure padding, at C = 1024 and C = 768.
Per case:
  * position independence: the remainder's token columns copied to the front of a second input give bit-equal plane rows there;
  * float64 LayerNorm per token class within the bound tests/test_gpu_layernorm_planes.py holds this kernel to (reference_bounds:
    the larger of 2 x ATen's f32 error and 1.25 x the numpy f32 model of the kernel's summation order, + 2^-22; tests/test_gpu_split.py
    compares this entry between the two binaries, bit for bit, and holds no float64 bound of its own);
  * rows past the last computed block are zero, planes are well formed, the status word is 0."""
import ctypes

import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from test_gpu_layernorm_planes import EPS, bits, reference_bounds

pytestmark = [pytest.mark.gpu, pytest.mark.probes]
DEV = "cuda"


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def ln_planes_live(x_tm, gamma, beta, live):
    """gp_layernorm_planes on x_tm [Mpad][C] (CPU, token-major) with `live` token rows -> planes (hi, lo) [Mpad][C] on the CPU,
    pre-filled with a NaN pattern so that an unwritten row shows."""
    Mpad, C = x_tm.shape
    X = x_tm.to(DEV).t().contiguous()
    hi = torch.full((Mpad, C), float("nan"), dtype=torch.float16, device=DEV)
    lo = torch.full_like(hi, float("nan"))
    g, b = gamma.to(DEV), beta.to(DEV)
    lib = _lib.lib()
    try:
        lib.gp_vit_set_ln_live(ctypes.c_int(live))
        _lib.call("gp_layernorm_planes", _lib.ptr(X), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(g), _lib.ptr(b), _lib.i(C), _lib.i(Mpad), _lib.f(EPS),
                  _lib.stream_ptr())
        torch.cuda.synchronize()
    finally:
        lib.gp_vit_set_ln_live(ctypes.c_int(0))
    return hi.cpu(), lo.cpu()


# (tag, live tokens as a function of the slot count S, Mpad - round_up(live, 64) in rows): remainder = ceil(live / 32) mod S
CASES = [("rem1+pad", lambda S: 32 * (S + 1), 0),          # Mpad = 32 (S + 2): one block of pure padding behind one remainder block
         ("rem2", lambda S: 32 * (S + 2), 0),              # the 64-crop shape: no padding at all
         ("rem2-partial+pad", lambda S: 32 * (S + 1) + 5, 192),   # last block holds 5 tokens; 27 + 192 rows of padding
         ("none", lambda S: 32 * S, 0),                    # a whole round: the plain kernel, every row computed
         ("none+pad", lambda S: 32 * S - 7, 128)]          # plain kernel, a partial last block and four blocks that do not run


# C = 768 (six chunks, an extra token's third hundred channels on half the threads) runs the folded cases and one plain case
PARAMS = [(1024,) + c for c in CASES] + [(768,) + c for c in CASES if c[0] in ("rem2", "rem2-partial+pad", "none+pad")]


@pytest.mark.parametrize("C,tag,live_of,extra_pad", PARAMS, ids=[f"{p[0]}-{p[1]}" for p in PARAMS])
def test_layernorm_tail(C, tag, live_of, extra_pad):
    S = slots()
    live = live_of(S)
    Mpad = (live + 63) // 64 * 64 + extra_pad
    nblk = (live + 31) // 32
    rem = nblk % S
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, 300 + C + Mpad)
    hi, lo = ln_planes_live(x, gamma, beta, live)
    _lib.check_status()   # the status word is 0
    # rows the launch computes: all live tokens; (plain path) the rest of the last block
    assert sr.planes_well_formed(hi[:live], lo[:live]), tag
    top = live if 1 <= rem <= 4 else nblk * 32
    assert not bool(bits(hi[top:]).ne(0).any()) and not bool(bits(lo[top:]).ne(0).any()), f"{tag}: rows from {top} on must be zero planes"
    # float64, per token class, over the live rows
    y, xhat, ref, model, bound = reference_bounds(x[:live], cls[:live], gamma, beta, 16, False)
    got = sr.per_class_max(sr.layernorm_error(sr.planes_value(hi[:live], lo[:live], 8.0), y, xhat, gamma, beta), cls[:live])
    for k in got:
        print(f"LN tail {tag} C={C} S={S} live={live} Mpad={Mpad} (blocks {nblk} = {nblk // S} x {S} + {rem}) class {k:8s}: kernel {got[k]:.3e}  "
              f"bound {bound[k]:.3e}  (f32 CPU reference {ref[k]:.3e}, numpy f32 model {model[k]:.3e})")
        assert got[k] <= bound[k], (tag, k, got[k], bound[k])
    # position independence: the tokens behind the last whole round, moved to the front (first-round positions, other lanes)
    first = (nblk - rem) * 32 if rem else live - 40
    n = live - first
    x2 = x.clone()
    x2[:n] = x[first:live]
    hi2, lo2 = ln_planes_live(x2, gamma, beta, live)
    _lib.check_status()
    assert torch.equal(bits(hi2[:n]), bits(hi[first:live])) and torch.equal(bits(lo2[:n]), bits(lo[first:live])), \
        f"{tag}: the planes of tokens {first}..{live - 1} depend on where they sit"
    assert torch.equal(bits(hi2[n:first]), bits(hi[n:first])) and torch.equal(bits(lo2[n:first]), bits(lo[n:first]))
