"""GPU: the ViT's last kernel writing the split matcher's query planes itself (gp_vit.hip: features_planes_kernel, selected by
gp_vit_forward_split2's normalize == 2; Dinov2ViT.patch_features(matcher_planes=True), AENet.forward_planes) against the two
kernels it replaces in GigaPose.predict -- features_kernel (normalize = 1) followed by l2norm_split_kernel (matching.normalize_split):

  * bit-equal hi / lo planes and patch masks at ViT-S x 1, 3, 17 crops (odd B puts a crop's first patch column b * 257 + 1 on every
    alignment; 17 is above features_kernel's chunk-count threshold at 16) and at width 1024 x 2 crops (the 64 KB LDS block);
  * against a float64 restatement of the double normalisation (F.normalize over C, the matcher's F.normalize again, x 32): the fused
    planes may be no further from it than the unfused path's planes on the same inputs (both figures printed; bit-equal planes make
    them the same number);
  * padding crops (live_rows) get all-zero planes; a non-finite residual stream raises the status bit it raises today."""
import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_amd.matching import normalize_split, patch_masks
from gigapose_amd.vit import Dinov2ViT
from gigapose_testing import factory
from gigapose_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def make_vit(dim, depth, seed):
    return syn.fill_state_dict(Dinov2ViT(dim, depth, dim // 64), seed).eval().to(DEV).set_numerics("split")


def crops(seed, B):
    rs = np.random.RandomState(seed)
    img = torch.from_numpy(rs.standard_normal((B, 3, 224, 224)).astype(np.float32)).to(DEV)
    mask = torch.from_numpy((rs.uniform(size=(B, 224, 224)) < 0.6).astype(np.float32)).to(DEV)
    return img, mask


def both_paths(vit, img, mask):
    """-> (hi, lo, masks) of the unfused path (parent code), the same of the fused path, the raw features (B, C, 256)."""
    B = img.shape[0]
    feat = vit.patch_features(img, normalize=True, stop_after_layers=1)
    unfused = normalize_split(feat.reshape(B, vit.dim, 256), mask)
    planes = vit.patch_features(img, stop_after_layers=1, matcher_planes=True)
    fused = (planes[0], planes[1], patch_masks(mask))
    raw = vit.patch_features(img, normalize=False, stop_after_layers=1).reshape(B, vit.dim, 256)
    torch.cuda.synchronize()
    _lib.check_status()
    return unfused, fused, raw


def restated(raw):
    """float64: F.normalize over C (eps 1e-12) twice, x 32 -> (B, 256, C)."""
    x = raw.double().cpu().numpy()
    v = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    w = v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12) * 32.0
    return w.transpose(0, 2, 1)


def check(vit, B, seed):
    img, mask = crops(seed, B)
    unfused, fused, raw = both_paths(vit, img, mask)
    assert fused[0].shape == (B, 256, vit.dim) and fused[0].dtype == torch.float16
    ref = restated(raw)
    err = [np.abs(hi.double().cpu().numpy() + lo.double().cpu().numpy() - ref).max() for hi, lo, _ in (unfused, fused)]
    print(f"features -> planes, C={vit.dim} B={B}: max |planes - float64| (of values up to 32) unfused {err[0]:.3e}, fused {err[1]:.3e}")
    assert np.isfinite(ref).all() and np.abs(ref).max() > 1.0
    for name, a, b in zip(("hi", "lo", "patch masks"), unfused, fused):
        assert torch.equal(a, b), f"{name} differ from features_kernel + l2norm_split_kernel"
    assert err[1] <= err[0]   # the tolerance is the unfused path's own error on these inputs


@pytest.fixture(scope="module")
def vit_s():
    return make_vit(384, 2, 11)


@pytest.mark.parametrize("B", [1, 3, 17])
def test_planes_equal_the_unfused_path_vit_s(vit_s, B):
    check(vit_s, B, 20 + B)


def test_planes_equal_the_unfused_path_width_1024():
    check(make_vit(1024, 1, 12), 2, 31)


def test_padding_rows_get_zero_planes():
    model = factory.build_model("dinov2_vits14", k=4, device=DEV, seed=3, numerics="split")
    img, _ = crops(41, 4)
    img[2:] = 0
    out = model._backbone_rows("ae_planes", model.ae_net.forward_planes, img, 2, row_dim=1)
    live = model.ae_net.forward_planes(img[:2])
    torch.cuda.synchronize()
    _lib.check_status()
    assert out.shape == (2, 4, 256, 384) and out.dtype == torch.float16
    assert torch.equal(out[:, :2], live) and bool(live.ne(0).any())
    assert not bool(out[:, 2:].view(torch.int16).ne(0).any()), "padding crops must get all-zero planes"
    # an all-padding batch does not run the network and keeps the shape
    none = model._backbone_rows("ae_planes", model.ae_net.forward_planes, img, 0, row_dim=1)
    assert none.shape == out.shape and not bool(none.view(torch.int16).ne(0).any())


def test_non_finite_residual_stream_raises_the_same_status_bit(vit_s):
    img, _ = crops(51, 3)
    img[1, 0, 100, 37] = float("nan")
    vit_s.patch_features(img, normalize=True, stop_after_layers=1)
    torch.cuda.synchronize()
    want = _lib.take_status()
    vit_s.patch_features(img, stop_after_layers=1, matcher_planes=True)
    torch.cuda.synchronize()
    got = _lib.take_status()
    print(f"status bits with a NaN pixel: unfused 0x{want:x}, fused 0x{got:x}")
    assert want & 4 and got == want
