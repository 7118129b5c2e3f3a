"""GPU parity: k-major f32 MFMA GEMM (bit-exact vs the oracle's fmaf chain) and the HIP DINOv2
forward vs the numpy restatement and the HF Dinov2Model stand-in (floating point: tolerance)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cpu as oracle
from oracle import vit_numpy
from test_oracle_vit import hf_model, sd_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda"


def view_ptr(t):
    """Device pointer of a view (a window of a wider array is not contiguous: _lib.ptr refuses it)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def laid_out_kmajor(A, B, epi, res, layout):
    """The operand windows and output buffers of a gp_gemm_kmajor(_sk) launch under gigapose_testing.gemm_layout.Layout."""
    from gigapose_testing import gemm_layout as gl

    K, I = A.shape
    J = B.shape[1]
    tA = gl.embed(torch.from_numpy(A).to(DEV), layout.a_ld or I, layout.a_col)[1]
    tB = gl.embed(torch.from_numpy(B).to(DEV), layout.b_ld or J, layout.b_col)[1]
    flat, D, tr, ldr, pair = gl.place_output(layout, I, J, epi, None if res is None else torch.from_numpy(res).to(DEV), DEV)
    return tA, tB, flat, D, tr, ldr, pair


def hip_gemm(A, B, epi=0, bias=None, scale=None, res=None, layout=None):
    """layout (gigapose_testing.gemm_layout.Layout): operands as windows of NaN-filled arrays, D inside a sentinel-filled buffer; returns
    (that buffer, (residual array after, before) or None) on the device for gemm_layout.check instead of D."""
    from gigapose_amd import _lib

    K, I = A.shape
    J = B.shape[1]
    tb = None if bias is None else torch.from_numpy(bias).to(DEV)
    ts = None if scale is None else torch.from_numpy(scale).to(DEV)
    if layout is not None:
        tA, tB, flat, D, tr, ldr, pair = laid_out_kmajor(A, B, epi, res, layout)
        _lib.call("gp_gemm_kmajor", view_ptr(tA), _lib.i(tA.stride(0)), view_ptr(tB), _lib.i(tB.stride(0)), view_ptr(D), _lib.i(D.stride(0)),
                  _lib.i(I), _lib.i(J), _lib.i(K), _lib.i(epi), _lib.ptr(tb), _lib.ptr(ts), view_ptr(tr), _lib.i(ldr), _lib.stream_ptr())
        torch.cuda.synchronize()
        return flat, pair
    tA, tB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    D = torch.empty(I, J, device=DEV)
    tr = None if res is None else torch.from_numpy(res).to(DEV)
    _lib.call("gp_gemm_kmajor", _lib.ptr(tA), _lib.i(I), _lib.ptr(tB), _lib.i(J), _lib.ptr(D), _lib.i(J),
              _lib.i(I), _lib.i(J), _lib.i(K), _lib.i(epi), _lib.ptr(tb), _lib.ptr(ts), _lib.ptr(tr), _lib.i(J),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return D.cpu().numpy()


@pytest.mark.parametrize("epi", [0, 1, 3, 4, 5])
def test_gemm_bit_exact_vs_fmaf_chain(epi):
    rs = np.random.RandomState(40 + epi)
    I, J, K = 256, 384, 80          # asymmetric everything: catches transposes / tile swaps
    A = rs.standard_normal((K, I)).astype(np.float32)
    B = rs.standard_normal((K, J)).astype(np.float32)
    bias = rs.standard_normal(J if epi == 4 else I).astype(np.float32)
    scale = rs.standard_normal(I).astype(np.float32)
    res = rs.standard_normal((I, J)).astype(np.float32)
    got = hip_gemm(A, B, epi, bias, scale, res)
    ref = oracle.gemm_kmajor(A, B, epi, bias, scale, res)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    np.testing.assert_allclose(got if epi == 0 else got, ref, rtol=1e-6)


def hip_gemm_sk(A, B, epi, bias, scale, res, layout=None):
    """gp_gemm_kmajor_sk: same contraction with the stream-K scratch (tile count not a multiple of the slots).  layout: as hip_gemm's."""
    import ctypes
    from gigapose_amd import _lib

    lib = _lib.lib()
    nbytes = lib.gp_gemm_streamk_workspace_bytes()
    K, I = A.shape
    J = B.shape[1]
    tb, ts = torch.from_numpy(bias).to(DEV), torch.from_numpy(scale).to(DEV)
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    _lib.call("gp_gemm_streamk_reset", _lib.ptr(ws), _lib.stream_ptr())
    _lib.status_word(DEV).zero_()
    if layout is not None:
        tA, tB, flat, D, tr, ldr, pair = laid_out_kmajor(A, B, epi, res, layout)
    else:
        tA, tB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
        D = torch.from_numpy(res).to(DEV).clone() if epi == 3 else torch.empty(I, J, device=DEV)
        tr, ldr = (D if epi == 3 else None), J       # in-place residual, as the ViT uses it
    for _ in range(2):                               # second launch: flags of the first must not satisfy it
        if epi == 3 and tr is D:
            D.copy_(torch.from_numpy(res))
        _lib.call("gp_gemm_kmajor_sk", view_ptr(tA), _lib.i(tA.stride(0)), view_ptr(tB), _lib.i(tB.stride(0)), view_ptr(D), _lib.i(D.stride(0)),
                  _lib.i(I), _lib.i(J), _lib.i(K), _lib.i(epi), _lib.ptr(tb), _lib.ptr(ts), view_ptr(tr), _lib.i(ldr),
                  _lib.ptr(ws), ctypes.c_size_t(nbytes), _lib.stream_ptr())
    if hasattr(lib, "gp_gemm_streamk_error"):        # the scratch's error word: its reader is in the probe library only
        assert lib.gp_gemm_streamk_error(_lib.ptr(ws), _lib.stream_ptr()) == 0, "a stream-K hand-off timed out"
    torch.cuda.synchronize()
    _lib.check_status()                              # both builds: GP_STATUS_HANDOFF_CHAIN
    if layout is not None:
        return flat, pair
    return D.cpu().numpy()


@pytest.mark.probes
@pytest.mark.parametrize("shape", ["proj", "v", "qk", "ragged", "fc1"])
def test_gemm_streamk_is_bit_identical(shape):
    """ViT-L shapes at B=64 (8 x 129, 129 x 8, 16 x 129 tiles on 1024 resident slots) + a tile count with
    T % 8 != 0: tiles split between two workgroups are handed over as accumulator fragments; the result must
    depend neither on the split nor on the tile order, and equal the oracle's fmaf chain bit for bit."""
    from gigapose_amd import _lib

    rs = np.random.RandomState(7)
    I, J, K, epi = {"proj": (1024, 129 * 128, 80, 3), "v": (129 * 128, 1024, 48, 4), "qk": (2048, 129 * 128, 32, 1),
                    "ragged": (9 * 128, 115 * 128, 64, 0), "fc1": (4096, 129 * 128, 32, 1)}[shape]
    A = rs.standard_normal((K, I)).astype(np.float32)
    B = rs.standard_normal((K, J)).astype(np.float32)
    bias = rs.standard_normal(J if epi == 4 else I).astype(np.float32)
    scale = rs.standard_normal(I).astype(np.float32)
    res = rs.standard_normal((I, J)).astype(np.float32)
    lib = _lib.lib()
    lib.gp_gemm_set_streamk(2)   # also where the built-in rule would not split (fc1: several whole tiles per slot)
    try:
        split = hip_gemm_sk(A, B, epi, bias, scale, res)
    finally:
        lib.gp_gemm_set_streamk(1)
    lib.gp_gemm_set_group(3)
    try:
        plain = hip_gemm(A, B, epi, bias, scale, res)   # one workgroup per tile, other tile order
    finally:
        lib.gp_gemm_set_group(8)
    np.testing.assert_array_equal(split.view(np.uint32), plain.view(np.uint32))
    rows = np.r_[0:40, I // 2:I // 2 + 24, I - 40:I]     # oracle on a band of rows
    ref = oracle.gemm_kmajor(np.ascontiguousarray(A[:, rows]), B, epi, bias if epi == 4 else bias[rows], scale[rows], res[rows])
    np.testing.assert_array_equal(split[rows].view(np.uint32), ref.view(np.uint32))


def test_gemm_gelu_and_errors():
    from gigapose_amd import _lib

    rs = np.random.RandomState(50)
    A = rs.standard_normal((32, 128)).astype(np.float32)
    B = rs.standard_normal((32, 128)).astype(np.float32)
    bias = rs.standard_normal(128).astype(np.float32)
    got = hip_gemm(A, B, 2, bias)
    ref = torch.nn.functional.gelu(torch.from_numpy((A.T.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
                                                    + bias[:, None])).numpy()
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6)
    with pytest.raises(_lib.GigaPoseHipError):
        hip_gemm(A[:, :100].copy(), B)  # I not a multiple of 128


def run_vit(dim, depth, heads, B, seed, stop=None):
    from gigapose_amd.vit import Dinov2ViT

    hf = hf_model(dim, depth, heads, seed=seed)
    vit = Dinov2ViT.from_hf(hf).to(DEV)
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed + 1))
    return hf, vit, x


@pytest.mark.parametrize("stop", [0, 1, 2])
def test_vit_layerwise_small(stop):
    """dim 128 / depth 2: embeddings only, one block, two blocks -- localises any layout bug."""
    hf, vit, x = run_vit(128, 2, 2, 3, seed=60)
    got = vit.patch_features(x.to(DEV), normalize=False, stop_after_layers=stop).cpu().numpy()
    ref = vit_numpy.patch_features(sd_numpy(vit.cpu()), x.numpy(), 2, 2, normalize=False, stop_after_layers=stop)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=3e-5)


def test_vit_small_s14_vs_hf_and_numpy():
    """ViT-S/14 (BASELINE config 1 backbone), B=3 (Mpad padding exercised: 771 -> 896)."""
    torch.set_num_threads(max(1, torch.get_num_threads()))
    hf, vit, x = run_vit(384, 12, 6, 3, seed=70)
    feats = vit.patch_features(x.to(DEV)).cpu()
    xp = vit.forward_features(x.to(DEV))["x_prenorm"].cpu()
    with torch.no_grad():
        ref = hf(pixel_values=x, output_hidden_states=True).hidden_states[-1]
    np.testing.assert_allclose(xp.numpy(), ref.numpy(), rtol=2e-4, atol=1e-4)
    ref_f = torch.nn.functional.normalize(ref[:, 1:].permute(0, 2, 1), dim=1).reshape(3, 384, 16, 16)
    np.testing.assert_allclose(feats.numpy(), ref_f.numpy(), rtol=0, atol=2e-5)
    ref_np = vit_numpy.patch_features(sd_numpy(vit.cpu()), x.numpy(), 12, 6)
    np.testing.assert_allclose(feats.numpy(), ref_np, rtol=0, atol=2e-5)


def test_vit_large_l14_vs_hf():
    """ViT-L/14 (the north-star backbone), B=2, against HF on the host CPU."""
    hf, vit, x = run_vit(1024, 24, 16, 2, seed=80)
    feats = vit.patch_features(x.to(DEV)).cpu()
    with torch.no_grad():
        ref = hf(pixel_values=x, output_hidden_states=True).hidden_states[-1]
    ref_f = torch.nn.functional.normalize(ref[:, 1:].permute(0, 2, 1), dim=1).reshape(2, 1024, 16, 16)
    np.testing.assert_allclose(feats.numpy(), ref_f.numpy(), rtol=0, atol=3e-5)
    # chunking / batch-size independence: same crop alone gives the same features bit-for-bit
    one = vit.to(DEV).patch_features(x[:1].to(DEV)).cpu()
    np.testing.assert_array_equal(one.numpy().view(np.uint32), feats[:1].numpy().view(np.uint32))


def test_aenet_interface_chunks():
    from gigapose_amd.ae_net import AENet

    hf, vit, x = run_vit(128, 2, 2, 5, seed=90)
    net = AENet("dinov2_vits14", vit.to(DEV), descriptor_size=128, max_batch_size=2)
    a = net(x.to(DEV))
    b = vit.patch_features(x.to(DEV))
    assert tuple(a.shape) == (5, 128, 16, 16)
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert tuple(net(x[:0].to(DEV)).shape) == (0, 128, 16, 16)


def test_vit_large_width_every_batch_size_split_vs_chain():
    """ViT-L width (4 blocks) at batch sizes on both sides of every path switch of the split numerics: 1-7 crops (fewer than 8 plane
    tiles: 128 x 128 kernels), 8-63 (plane GEMMs with the parallel split-K, S = 16 ... 1 slots per tile, strips of B rows), 64 and
    65 (serial kernel, ragged strip) -- the unit-norm features must agree with the bit-exact chain mode to f32 round-off at every
    size, and a crop's features must not depend on the batch it is in beyond that."""
    import numpy as np

    from gigapose_amd import _lib
    from gigapose_testing import synthetic as syn
    from gigapose_amd.vit import Dinov2ViT

    vit = syn.fill_state_dict(Dinov2ViT(1024, 4, 16), 21).eval().to(DEV)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((65, 3, 224, 224)).astype(np.float32)).to(DEV)
    ref = vit.set_numerics("chain").patch_features(x[:16]).clone()          # chain: independent of the batch composition, bit for bit
    assert torch.equal(vit.patch_features(x[:3]), ref[:3])
    vit.set_numerics("split")
    worst = 0.0
    for B in (1, 2, 3, 5, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 65):
        f = vit.patch_features(x[:B])
        torch.cuda.synchronize()
        _lib.check_status()
        n = min(B, 16)
        d = (f[:n] - ref[:n]).abs().max().item()
        worst = max(worst, d)
        assert torch.isfinite(f).all() and d < 2e-6, f"B={B}: split vs chain {d:.2e}"
    print(f"ViT-L width, B = 1 .. 65: max |split - chain| over unit-norm features {worst:.2e}")


@pytest.mark.parametrize("numerics", ["split", "chain"])
def test_vit_large_with_peaked_attention_vs_float64(numerics):
    """A random-init ViT's softmax is nearly uniform (logit std 0.4), so the ViT-level comparisons above cannot see attention errors
    (missing 5).  Here the HF stand-in's query / key weights are scaled x 3 -- logit std ~ 3.7, most of a row's mass on a
    few keys, as in a trained DINOv2 -- and the whole ViT-L forward at 64 crops (split: the plane path with attention_split_kernel;
    chain: the f32 kernels) is compared with the SAME network evaluated in float64 (torch on the GPU), next to torch's own f32 forward."""
    from gigapose_amd.vit import Dinov2ViT

    B = 64 if numerics == "split" else 8
    hf = hf_model(1024, 24, 16, seed=90)
    with torch.no_grad():
        for layer in hf.encoder.layer:
            layer.attention.attention.query.weight.mul_(3.0)
            layer.attention.attention.key.weight.mul_(3.0)
    vit = Dinov2ViT.from_hf(hf).to(DEV)
    vit.set_numerics(numerics)
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(91)).to(DEV)
    mine = vit.patch_features(x).double()
    hf = hf.to(DEV)
    try:
        hf.config._attn_implementation = "eager"
    except Exception:
        pass
    with torch.no_grad():
        r32 = hf(pixel_values=x, output_hidden_states=True).hidden_states[-1]
        hf64 = hf.double()
        out = hf64(pixel_values=x.double(), output_hidden_states=True, output_attentions=True)
        r64 = out.hidden_states[-1]
        att = out.attentions[12] if out.attentions is not None else None

    def unit(h):
        return torch.nn.functional.normalize(h[:, 1:].permute(0, 2, 1), dim=1).reshape(B, 1024, 16, 16)

    f64, f32 = unit(r64), unit(r32.double())
    e_m, e_r = (mine - f64).abs(), (f32 - f64).abs()
    rms = lambda e: float((e ** 2).mean().sqrt())
    ent = float(-(att * att.clamp_min(1e-300).log()).sum(-1).mean()) if att is not None else float("nan")
    top = float(att.max(-1).values.mean()) if att is not None else float("nan")
    print(f"ViT-L [{numerics}], {B} crops, query / key weights x 3 (layer-12 attention: mean entropy {ent:.2f} of {np.log(257):.2f}, mean top weight {top:.3f}): "
          f"unit-norm features vs float64 (rms {rms(f64):.3e}): ours max {float(e_m.max()):.2e} rms {rms(e_m):.2e} | torch f32 (GPU) max {float(e_r.max()):.2e} rms {rms(e_r):.2e}")
    from gigapose_amd import _lib
    _lib.check_status()
    assert ent != ent or ent < 4.5, "the attention is not peaked: the test would not see attention errors"
    assert rms(e_m) < 2.0 * rms(e_r) + 1e-8 and float(e_m.max()) < 4e-6
