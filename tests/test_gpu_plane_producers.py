"""GPU: the plane producers bit for bit -- gp_split_planes, gp_planes_from_cm and the planes gp_l2norm_split_mask writes.

gp_split_planes is the TOOL every plane test builds its inputs with (several compute their float64 reference on the plane values it
made, which makes them blind to it); gp_planes_from_cm only runs when a ResNet's stem does not fit the split stem.  The host
restatement (gigapose_testing/stage_refs.py: split_planes_host; tests/test_stage_refs.py) is v = f32(s x), hi = f16(v), lo = f16(v -
f32(hi)) in round-to-nearest-even.  split_planes_kernel keeps a compiler barrier between the multiply and the conversion because the
compiler otherwise folds both into one instruction (one rounding instead of two: hi and lo would see different v); the other producers
rely on their scale being a power of two.  Only a bit-exact comparison notices if either stops holding."""
import ctypes

import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def bits(t):
    return t.cpu().view(torch.int16)


def assert_same_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} f16 words differ; first at {i}: got 0x{int(g[i]) & 0xffff:04x}, "
                             f"expected 0x{int(w[i]) & 0xffff:04x}")


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000003])
@pytest.mark.parametrize("scale", [8.0, 64.0, 0.25, 1.0, 3.3])
def test_split_planes_bit_exact(scale, count):
    """Counts around the 256-thread block and a large ragged one; values 1e-30 .. 8000 of both signs, +-0, exact f16 values, halfway
    cases, f16-subnormal lows; scales: powers of two and 3.3 (what the barrier exists for).  Two guard words behind the buffers stay
    untouched (the last block is partial)."""
    x = torch.from_numpy(sr.split_values_case(count, 1000 + count))
    want_hi, want_lo = sr.split_planes_host(x, scale)
    xd = x.to(DEV)
    hi = torch.full((count + 2,), -7.0, dtype=torch.float16, device=DEV)
    lo = torch.full((count + 2,), -7.0, dtype=torch.float16, device=DEV)
    _lib.call("gp_split_planes", _lib.ptr(xd), ctypes.c_size_t(count), _lib.f(scale), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert_same_bits(hi[:count], want_hi, f"gp_split_planes hi, scale {scale}, count {count}")
    assert_same_bits(lo[:count], want_lo, f"gp_split_planes lo, scale {scale}, count {count}")
    assert hi[count:].tolist() == [-7.0, -7.0] and lo[count:].tolist() == [-7.0, -7.0]
    _lib.check_status()


@pytest.mark.parametrize("C,npix", [(128, 12544 * 3), (72, 1000), (33, 31), (1, 1)])
def test_planes_from_cm_bit_exact(C, npix):
    """[C][npix] f32 -> planes [npix][C] of 8 x: the conversion and the 32 x 32 LDS transpose, whole tiles and ragged ones in both directions."""
    rs = np.random.RandomState(C + npix)
    x = torch.from_numpy((rs.standard_normal((C, npix)) * 10.0 ** rs.uniform(-6, 2, (C, npix))).astype(np.float32))
    x.reshape(-1)[: min(C * npix, 22)] = torch.from_numpy(sr.split_values_case(23, 3)[1:1 + min(C * npix, 22)])
    want_hi, want_lo = sr.split_planes_host(x.t().contiguous(), 8.0)
    hi = torch.full((npix * C + 2,), -7.0, dtype=torch.float16, device=DEV)
    lo = torch.full((npix * C + 2,), -7.0, dtype=torch.float16, device=DEV)
    _lib.call("gp_planes_from_cm", _lib.ptr(x.to(DEV)), _lib.i(C), _lib.i(npix), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert_same_bits(hi[:npix * C], want_hi, f"gp_planes_from_cm hi ({C}, {npix})")
    assert_same_bits(lo[:npix * C], want_lo, f"gp_planes_from_cm lo ({C}, {npix})")
    assert hi[npix * C:].tolist() == [-7.0, -7.0] and lo[npix * C:].tolist() == [-7.0, -7.0]
    _lib.check_status()


def test_planes_from_cm_range_guard():
    """8 x 8100 = 64800 fits f16 (clean), 8 x 8200 = 65600 does not: GP_STATUS_SPLIT_RANGE_CONV, a status bit."""
    x = torch.zeros(72, 1000)
    x[5, 999] = -8100.0
    hi = torch.zeros(1000, 72, dtype=torch.float16, device=DEV)
    lo = torch.zeros_like(hi)
    _lib.call("gp_planes_from_cm", _lib.ptr(x.to(DEV)), _lib.i(72), _lib.i(1000), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())
    torch.cuda.synchronize()
    _lib.check_status()
    assert float(hi[999, 5]) + float(lo[999, 5]) == -64800.0
    x[5, 999] = 8200.0
    _lib.call("gp_planes_from_cm", _lib.ptr(x.to(DEV)), _lib.i(72), _lib.i(1000), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _lib.take_status() == 16
    for bad in (dict(C=0), dict(npix=0), dict(X=None)):
        kw = dict(X=x.to(DEV), C=72, npix=1000)
        kw.update(bad)
        with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_planes_from_cm"):
            _lib.call("gp_planes_from_cm", _lib.ptr(kw["X"]), _lib.i(kw["C"]), _lib.i(kw["npix"]), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())


@pytest.mark.parametrize("C", [48, 384, 1024])
def test_l2norm_split_planes_are_the_split_of_the_chain_normalisation(C):
    """gp_l2norm_split_mask's planes == split(32 q) bit for bit, q = gp_l2norm_cp's output on the same input (the same fma chain for the
    norm and the same division; q itself is pinned bit for bit to oracle.cpu.l2norm_cp elsewhere); padded channels are zero."""
    from gigapose_amd.matching import normalize_split

    rs = np.random.RandomState(C)
    rows = 5
    x = torch.from_numpy((rs.standard_normal((rows, C, 256)) * rs.uniform(0.1, 30, (rows, 1, 256))).astype(np.float32)).to(DEV)
    q = torch.empty_like(x)
    _lib.call("gp_l2norm_cp", _lib.ptr(x), _lib.ptr(q), _lib.i(rows), _lib.i(C), _lib.stream_ptr())
    hi, lo = normalize_split(x)
    torch.cuda.synchronize()
    Cp = (C + 31) // 32 * 32
    assert hi.shape == (rows, 256, Cp) and lo.shape == hi.shape
    want_hi, want_lo = sr.split_planes_host(q.cpu().transpose(1, 2).contiguous(), 32.0)
    assert_same_bits(hi[..., :C].contiguous(), want_hi, f"l2norm_split hi, C = {C}")
    assert_same_bits(lo[..., :C].contiguous(), want_lo, f"l2norm_split lo, C = {C}")
    assert bool((bits(hi[..., C:].contiguous()) == 0).all()) and bool((bits(lo[..., C:].contiguous()) == 0).all())
    # the unit vectors themselves: f32-exact normalisation (norm of q within a few ulp of 1)
    assert float((q.double().pow(2).sum(1).sqrt() - 1.0).abs().max()) < 1e-6
    _lib.check_status()
