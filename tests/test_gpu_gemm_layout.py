"""GPU: the five GEMM entry points under leading dimensions, base offsets and residuals other than the tight ones every stage test uses.

A laid-out launch runs the schedule of the tight launch of its shape, so its window must hold the tight result BIT FOR BIT (the tight
launches are held to float64 and the oracle in test_gpu_vit.py / test_gpu_split.py), and gigapose_testing.gemm_layout.check holds
everything around the window to what it was: sentinel-filled pad columns, columns of a plane row that belong to another launch, rows
beyond the strip, the words before the base, a residual that is not D; operands sit in NaN-filled arrays, so a read outside a window
shows as a NaN.  The plane cases use the product's own interleave (gp_vit.hip: q | k into columns 0 .. 2C, v into 2C .. 3C of one
[Mpad][3C] plane pair).  The last two tests run the plane GEMM at the largest outputs its byte-range guards accept (the first refused
sizes: tests/test_gemm_refusals_host.py)."""
import numpy as np
import pytest
import torch

from gigapose_testing import gemm_layout as gl
from test_gpu_split import (DEV, SPLIT256_SHAPES, also_on_probe_binary, binary_name, epilogue_f64, planes256_gemm, split256_case,
                            split256_gemm, split_gemm)
from test_gpu_vit import hip_gemm, hip_gemm_sk

pytestmark = pytest.mark.gpu

EPI3 = {"3-aliased": False, "3-separate": True}     # epilogue 3 with residual == D, and with a residual buffer of its own


def f32_layout(n_a, n_b, J, separate):
    """lda = width + 12 (window at column 8), ldb = width + 4 (window at column 4), D 4 floats into its buffer with ldd = J + 8, a
    separate residual with ldr = J + 4: every pointer stays 16-byte aligned, no two strides are equal."""
    return gl.Layout(a_ld=n_a + 12, a_col=8, b_ld=None if n_b is None else n_b + 4, b_col=0 if n_b is None else 4, d_ld=J + 8, d_base=4,
                     r_ld=J + 4 if separate else None)


def epi_of(case):
    return (3, EPI3[case]) if case in EPI3 else (case, False)


def check_f32(flat, pair, L, I, J, tight, what):
    gl.check(flat, gl.F32_SENTINEL, [(L.d_base, L.d_ld, I, J, torch.as_tensor(tight))], what=what, residual=pair)


def kmajor_case(I, J, K, epi, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((K, I)).astype(np.float32), rs.standard_normal((K, J)).astype(np.float32), epi,
            rs.standard_normal(J if epi == 4 else I).astype(np.float32), rs.standard_normal(I).astype(np.float32),
            rs.standard_normal((I, J)).astype(np.float32))


@also_on_probe_binary
@pytest.mark.parametrize("case", [0, 1, 4, "3-aliased", "3-separate"])
def test_kmajor_layout(case):
    epi, separate = epi_of(case)
    I, J, K = 256, 384, 80
    args = kmajor_case(I, J, K, epi, 140 + epi)
    tight = hip_gemm(*args)
    L = f32_layout(I, J, J, separate)
    flat, pair = hip_gemm(*args, layout=L)
    check_f32(flat, pair, L, I, J, tight, f"gp_gemm_kmajor epilogue {case}")


@also_on_probe_binary
@pytest.mark.parametrize("case", [0, "3-separate"])
def test_kmajor_streamk_layout(case):
    """The `ragged` shape of test_gemm_streamk_is_bit_identical (1035 tiles on 1024 slots: stream-K by the launcher's own rule), so tiles
    that were handed over as accumulator fragments store with the stride too."""
    epi, separate = epi_of(case)
    I, J, K = 9 * 128, 115 * 128, 64
    args = kmajor_case(I, J, K, epi, 7)
    tight = hip_gemm_sk(*args)
    L = f32_layout(I, J, J, separate)
    flat, pair = hip_gemm_sk(*args, layout=L)
    check_f32(flat, pair, L, I, J, tight, f"gp_gemm_kmajor_sk epilogue {case}")


@also_on_probe_binary
@pytest.mark.parametrize("act_is_b", [True, False])
@pytest.mark.parametrize("case", [1, 4, "3-aliased", "3-separate"])
def test_split_layout(case, act_is_b):
    epi, separate = epi_of(case)
    I, J, K = 256, 384, 96
    rs = np.random.RandomState(150 + epi)
    n_act, n_w = (J, I) if act_is_b else (I, J)
    act = rs.standard_normal((K, n_act)).astype(np.float32)
    W = (rs.standard_normal((n_w, K)) * 0.05).astype(np.float32)
    bias, scale = rs.standard_normal(J if epi == 4 else I).astype(np.float32), rs.standard_normal(I).astype(np.float32)
    res = rs.standard_normal((I, J)).astype(np.float32)
    tight = split_gemm(act, W, act_is_b, epi, bias, scale, res)
    L = f32_layout(n_act, None, J, separate)
    flat, pair = split_gemm(act, W, act_is_b, epi, bias, scale, res, layout=L)
    check_f32(flat, pair, L, I, J, tight, f"gp_gemm_split epilogue {case} act_is_b={act_is_b}")


@also_on_probe_binary
@pytest.mark.parametrize("shape", ["proj", "v"])
@pytest.mark.parametrize("case", [4, "3-separate"])
def test_split256_layout(case, shape):
    """The proj and v shapes of SPLIT256_SHAPES (260 tiles on 256 slots: every slot hands a partial tile over); one scratch serves the
    tight and the laid-out launch."""
    epi, separate = epi_of(case)
    I, J, K, _, act_is_b = SPLIT256_SHAPES[shape]
    act, W, bias_i, bias_j, scale, res = split256_case(shape)[:6]
    bias = bias_j if epi == 4 else bias_i
    from gigapose_amd import _lib

    ws = torch.full((_lib.lib().gp_gemm_split256_workspace_bytes() // 4,), float("nan"), device=DEV)
    tight = split256_gemm(act, W, act_is_b, epi, bias, scale, res, scratch=ws)
    L = f32_layout(act.shape[1], None, J, separate)
    flat, pair = split256_gemm(act, W, act_is_b, epi, bias, scale, res, layout=L, scratch=ws)
    check_f32(flat, pair, L, I, J, tight, f"gp_gemm_split256 {shape} epilogue {case}")


# ---- the plane GEMM

def planes_build(I, J, jv, epi):
    """Which build gp_gemm_planes256_launch takes (gp_plan256.h: gp_planes256_plan -- the ragged strip and the half-tile rule), 256 slots:
    tiled = the serial kernel on >= 256 tiles of 256 x 256; half-width = parallel split-K on 256 x 128 tiles (at most 128 whole tiles);
    whole = the parallel build without the reduction, one tile per slot (129-255 tiles, epilogues 3 and 7); split-K = the parallel
    split-K build on 256 x 256 tiles (what is left: epilogue 6 and the probe-only epilogues at 129-255 tiles)."""
    j_main = J if jv >= J else jv // 256 * 256
    tiles = (I // 256) * (j_main // 256)
    if tiles >= 256:
        return "tiled"
    if 2 * tiles <= 256 and epi in (3, 6, 7):
        return "half-width"
    return "whole" if epi in (3, 7) else "split-K"


def plane_inputs(I, J, jv, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(I, K, generator=g) * 0.05).to(DEV)
    Bm = (torch.randn(J, K, generator=g) * 1.3).to(DEV)
    Bm[(jv + 31) // 32 * 32:] = float("nan")          # rows beyond the strip are nobody's: reading one shows
    return A, Bm, torch.randn(I, generator=g).to(DEV), torch.randn(I, generator=g).to(DEV)


@also_on_probe_binary
@pytest.mark.parametrize("J,jv,K,builds", [(16640, 16448, 64, "tiled+strip | tiled+strip"),              # the B = 64 call
                                           (4352, 4112, 1024, "half-width+strip | half-width+strip"),    # B = 16
                                           (6400, 6168, 1024, "whole+strip | half-width+strip")])        # B = 24: 192 / 96 whole tiles
def test_planes_interleaved_outputs(J, jv, K, builds):
    """Launch A: I = 2048 into columns 0 .. 2048, launch B: I = 1024 (weights of its own) into columns 2048 .. 3072 of one sentinel-filled
    [J + 32][3072] plane pair, epilogue 7 -- q | k and v of ViT-L.  After A alone the columns from 2048 on still hold the sentinel; after
    both each window holds its tight launch and the rows from round_up(J_valid, 32) on the sentinel.  (4352, 4112) already takes the
    256 x 128 tiles for both widths, so the third shape is one whose wide launch takes the one-tile-per-slot build instead.)"""
    assert builds == " | ".join(planes_build(I, J, jv, 7) + "+strip" for I in (2048, 1024))
    rows, ldo = (jv + 31) // 32 * 32, 3072
    A1, Bm, b1, _ = plane_inputs(2048, J, jv, K, 11 + jv)
    A2, _, b2, _ = plane_inputs(1024, J, jv, K, 12 + jv)
    t1 = planes256_gemm(A1, Bm, 7, b1, j_valid=jv)
    t2 = planes256_gemm(A2, Bm, 7, b2, j_valid=jv)
    bufs = gl.place_planes(gl.Layout(o_ld=ldo), ldo, J, DEV)[:2]
    own1 = [[(0, ldo, rows, 2048, t[:rows])] for t in t1]
    own2 = [[(2048, ldo, rows, 1024, t[:rows])] for t in t2]
    planes256_gemm(A1, Bm, 7, b1, j_valid=jv, layout=gl.Layout(o_ld=ldo, o_col=0, o_bufs=bufs))
    for flat, sentinel, own, name in zip(bufs, (gl.F16_SENTINEL_HI, gl.F16_SENTINEL_LO), own1, ("out_hi", "out_lo")):
        gl.check(flat, sentinel, own, what=f"launch A alone, {name}")
    planes256_gemm(A2, Bm, 7, b2, j_valid=jv, layout=gl.Layout(o_ld=ldo, o_col=2048, o_bufs=bufs))
    for flat, sentinel, oa, ob, name in zip(bufs, (gl.F16_SENTINEL_HI, gl.F16_SENTINEL_LO), own1, own2, ("out_hi", "out_lo")):
        gl.check(flat, sentinel, oa + ob, what=f"launches A and B, {name}")


@also_on_probe_binary
def test_planes_gelu_output_with_a_stride():
    """Epilogue 6 at 192 whole tiles: the one plane build the interleave cases cannot reach with epilogue 7 (parallel split-K on
    256 x 256 tiles, reduced by the tile's owner), into columns 1024 .. 3072 of rows of 4096."""
    I, J, jv, K = 2048, 6400, 6168, 1024
    assert planes_build(I, J, jv, 6) == "split-K"
    rows, ldo = (jv + 31) // 32 * 32, 4096
    A, Bm, bias, _ = plane_inputs(I, J, jv, K, 31)
    tight = planes256_gemm(A, Bm, 6, bias, j_valid=jv)
    bufs = planes256_gemm(A, Bm, 6, bias, j_valid=jv, layout=gl.Layout(o_ld=ldo, o_col=1024))
    for flat, sentinel, t, name in zip(bufs, (gl.F16_SENTINEL_HI, gl.F16_SENTINEL_LO), tight, ("out_hi", "out_lo")):
        gl.check(flat, sentinel, [(1024, ldo, rows, I, t[:rows])], what=f"epilogue 6, {name}")


@also_on_probe_binary
@pytest.mark.parametrize("J,jv,K,build", [(16640, 16448, 64, "tiled"), (4352, 4112, 1024, "half-width"), (12544, 12336, 1024, "whole")])
def test_planes_f32_output_layout(J, jv, K, build):
    """Epilogue 3, I = 1024: D 4 floats into its buffer with ldd = J + 4 and a residual of its own with ldr = J + 8 (the columns from
    round_up(J_valid, 32) on keep the sentinel), then in place (those columns keep the residual).  (6400, 6168) would take the 256 x 128
    tiles like (4352, 4112); (12544, 12336), 48 crops, is the shape at which I = 1024 takes the one-tile-per-slot build."""
    I = 1024
    assert planes_build(I, J, jv, 3) == build
    cols = (jv + 31) // 32 * 32
    A, Bm, bias, scale = plane_inputs(I, J, jv, K, 21 + jv)
    res = torch.randn(I, J, generator=torch.Generator().manual_seed(jv)).to(DEV)
    tight = planes256_gemm(A, Bm, 3, bias, scale, res, j_valid=jv)
    assert torch.equal(tight[:, cols:], res[:, cols:])
    L = gl.Layout(d_base=4, d_ld=J + 4, r_ld=J + 8)
    flat, pair = planes256_gemm(A, Bm, 3, bias, scale, res, j_valid=jv, layout=L)
    gl.check(flat, gl.F32_SENTINEL, [(4, J + 4, I, cols, tight[:, :cols])], what=f"{build}, residual of its own", residual=pair)
    L = gl.Layout(d_base=4, d_ld=J + 4)
    flat, pair = planes256_gemm(A, Bm, 3, bias, scale, res, j_valid=jv, layout=L)
    gl.check(flat, gl.F32_SENTINEL, [(4, J + 4, I, J, tight)], what=f"{build}, in place")


# ---- the last addressable row: the largest outputs the byte-range guards accept (0x7ffffff0 bytes from the base, gp_split256.hip)

RSRC_BYTES = 0x7ffffff0


def need_free(gib):
    free = torch.cuda.mem_get_info()[0]
    assert free >= gib * 2 ** 30, f"{free / 2 ** 30:.1f} GiB free, the case needs {gib}"


@also_on_probe_binary
def test_planes_f32_output_at_the_last_addressable_row():
    """D of I = 1024 rows x the largest multiple-of-256 J with ((I - 1) ldd + J) * 4 <= 0x7ffffff0, K = 32, epilogue 3 with a residual of
    its own of the same size.  Rows 0 .. 47 and the last 48 rows against float64 within epilogue_f64's bound; no sentinel left in the
    last 256 rows (a store past what the buffer resource addresses is dropped without a fault)."""
    I, K = 1024, 32
    J = RSRC_BYTES // 4 // I // 256 * 256
    assert J == 524032 and ((I - 1) * J + J) * 4 <= RSRC_BYTES < ((I - 1) * (J + 256) + J + 256) * 4
    need_free(12)

    def run():
        g = torch.Generator().manual_seed(5)
        A = (torch.randn(I, K, generator=g) * 0.05).to(DEV)
        Bm = (torch.randn(J, K, generator=g) * 1.3).to(DEV)
        bias, scale = torch.randn(I, generator=g).to(DEV), torch.randn(I, generator=g).to(DEV)
        res = torch.randn(I, J, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        flat, pair = planes256_gemm(A, Bm, 3, bias, scale, res, layout=gl.Layout(d_ld=J, r_ld=J))
        D = gl.window(flat, 0, J, I, J)
        assert torch.equal(pair[0].view(torch.int32), pair[1].view(torch.int32)), "the residual was written"   # bits: its spare row is NaN
        rows = torch.cat([torch.arange(0, 48), torch.arange(I - 48, I)]).to(DEV)
        acc = A[rows].double() @ Bm.double().t()
        mag = A[rows].double().abs() @ Bm.double().abs().t()
        want, bound = epilogue_f64(3, acc, mag, bias[rows], scale[rows], res[rows])
        ratio = ((D[rows].double() - want).abs() / bound)
        print(f"[{binary_name()}] f32 D of {I} x {J} ({I * J * 4} bytes): max err / bound rows 0..47 {ratio[:48].max().item():.3f}, "
              f"last 48 rows {ratio[48:].max().item():.3f}")
        assert ratio.max().item() <= 1.0
        left = int((D[I - 256:] == gl.F32_SENTINEL).sum())
        assert left == 0, f"{left} elements of the last 256 rows were never written"

    try:
        run()
    finally:
        torch.cuda.empty_cache()


@also_on_probe_binary
def test_planes_plane_output_at_the_last_addressable_row():
    """Output planes of the largest multiple-of-256 J with ((J - 1) ldo + I) * 2 <= 0x7ffffff0 at I = ldo = 4096, K = 32, epilogue 7:
    the first and the last 256 token rows against float64 within the tolerance of test_planes256_gemm_epilogues (rtol = atol = 2e-5),
    and no sentinel left in them."""
    I, K = 4096, 32
    J = RSRC_BYTES // 2 // I // 256 * 256
    assert J == 261888 and ((J - 1) * I + I) * 2 <= RSRC_BYTES < ((J + 255) * I + I) * 2
    need_free(8)

    def run():
        g = torch.Generator().manual_seed(6)
        A = (torch.randn(I, K, generator=g) * 0.05).to(DEV)
        Bm = (torch.randn(J, K, generator=g) * 1.3).to(DEV)
        bias = torch.randn(I, generator=g).to(DEV)
        fhi, flo = planes256_gemm(A, Bm, 7, bias, layout=gl.Layout(o_ld=I))
        for name, lo, hi in (("first", 0, 256), ("last", J - 256, J)):
            oh, ol = gl.window(fhi, lo * I, I, 256, I), gl.window(flo, lo * I, I, 256, I)
            left = int((oh == gl.F16_SENTINEL_HI).sum()) + int((ol == gl.F16_SENTINEL_LO).sum())
            assert left == 0, f"{left} elements of the {name} 256 token rows were never written"
            want = Bm[lo:hi].double() @ A.double().t() + bias[None, :].double()
            got = (oh.double() + ol.double()) / 8.0
            ratio = ((got - want).abs() / (2e-5 + 2e-5 * want.abs())).max().item()
            print(f"[{binary_name()}] planes of {J} x {I} ({J * I * 2} bytes each): {name} 256 token rows max err / tolerance {ratio:.4f}")
            assert ratio <= 1.0
        assert bool((fhi[J * I:] == gl.F16_SENTINEL_HI).all()) and bool((flo[J * I:] == gl.F16_SENTINEL_LO).all()), "rows beyond J were written"

    try:
        run()
    finally:
        torch.cuda.empty_cache()
