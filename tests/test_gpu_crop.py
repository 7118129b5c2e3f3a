"""GPU parity: detection pre-processing kernels (gp_crop_resize_pad / gp_preprocess_detections) vs the reference
golden (tests/golden/crop.npz, written by the unmodified CropResizePad) and vs the numpy restatement on
randomised boxes; and vs ATen itself -- the reference's op chain run with torch ops on the CPU (gigapose_testing/crop_aten.py)
-- and a second golden of the reference (crop_sizes.npz) on the boxes at which the scale's two roundings and ATen's choice
between its two CPU kernels show.  Pixels and masks bit-exact; M's scale and constant entries bit-exact, its translations to
1 ulp (the reference's 3x3 matmul order is BLAS-defined)."""
import os

import numpy as np
import pytest
import torch

from gigapose_testing import crop_aten
from gigapose_testing import synthetic as syn
from oracle import crop_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(a).to(DEV)


def test_preprocess_matches_reference_golden(golden_dir):
    from gigapose_amd.crop import DetectionPreprocessor

    g = np.load(os.path.join(golden_dir, "crop.npz"))
    case = syn.detection_case(seed=int(g["seed"]))
    out = DetectionPreprocessor()(_t(case["rgb"]), _t(case["masks"]), _t(case["boxes"]), _t(case["im_id"]))
    np.testing.assert_array_equal(out["tar_mask"].cpu().numpy(), g["tar_mask"])
    np.testing.assert_array_equal(out["tar_img"].cpu().numpy().view(np.uint32), g["tar_img"].view(np.uint32))
    crop_aten.assert_M(out["tar_M"].cpu().numpy(), g["M"])


@pytest.mark.parametrize("seed,H,W,D", [(5, 480, 640, 40), (6, 97, 131, 25), (7, 1080, 1920, 12)])
def test_crop_resize_pad_equals_restatement_on_random_boxes(seed, H, W, D):
    from gigapose_amd.crop import CropResizePad

    case = syn.detection_case(seed=seed, n_img=1, D=D, H=H, W=W)
    rs = np.random.RandomState(seed)
    images = rs.standard_normal((D, 5, H, W)).astype(np.float32)     # C = 5: not tied to RGBA
    ref_img, ref_M = crop_numpy.crop_resize_pad(images, case["boxes"])
    out = CropResizePad(target_size=224)(_t(case["boxes"]), _t(images))
    np.testing.assert_array_equal(out["images"].cpu().numpy().view(np.uint32), ref_img.view(np.uint32))
    crop_aten.assert_M(out["M"].cpu().numpy(), ref_M)


def test_other_target_size_and_fused_equals_two_step():
    from gigapose_amd.crop import CLIP_MEAN, CLIP_STD, CropResizePad, DetectionPreprocessor

    case = syn.detection_case(seed=9, n_img=3, D=16, H=240, W=320)
    ref_img, ref_mask, ref_M = crop_numpy.preprocess_detections(case["rgb"], case["masks"], case["boxes"], case["im_id"],
                                                               target=112)
    out = DetectionPreprocessor(target_size=112)(_t(case["rgb"]), _t(case["masks"]), _t(case["boxes"]), _t(case["im_id"]))
    np.testing.assert_array_equal(out["tar_img"].cpu().numpy().view(np.uint32), ref_img.view(np.uint32))
    np.testing.assert_array_equal(out["tar_mask"].cpu().numpy(), ref_mask)
    crop_aten.assert_M(out["tar_M"].cpu().numpy(), ref_M)
    # the reference's own composition on the GPU: (rgb/255 * mask, mask) -> CropResizePad -> normalise
    # (host float32 arithmetic: torch's GPU division is not correctly rounded on ROCm builds)
    rgb = _t(case["rgb"].astype(np.float32) / np.float32(255.0))
    m = _t(case["masks"])
    rgba = torch.cat([rgb[_t(case["im_id"]).long()] * m[:, None], m[:, None]], dim=1)
    two = CropResizePad(target_size=112)(_t(case["boxes"]), rgba)
    mean = np.asarray(CLIP_MEAN, np.float32).reshape(3, 1, 1)
    std = np.asarray(CLIP_STD, np.float32).reshape(3, 1, 1)
    np.testing.assert_array_equal((two["images"][:, :3].cpu().numpy() - mean) / std, out["tar_img"].cpu().numpy())
    assert torch.equal(two["images"][:, 3], out["tar_mask"])


# ------------------------------------------------------------------------------ against ATen, at the sizes that carry the defects
@pytest.fixture(scope="module", params=[224, 37])
def aten_case(request):
    """The box list of crop_aten.gpu_boxes on one 97x131 frame, and ATen's result for both kernels' inputs, computed once."""
    from gigapose_amd.crop import CLIP_MEAN, CLIP_STD

    T = request.param
    case = crop_aten.gpu_case(T)
    H, W = crop_aten.GPU_FRAME
    case["T"] = T
    case["image5"] = crop_aten.index_image(H, W, C=5)                      # C = 5: not tied to RGBA
    case["ref_dense"] = crop_aten.aten_batch(case["image5"], case["boxes"], T)
    case["ref_fused"] = crop_aten.aten_preprocess_detections(case["rgb"], case["masks"], case["boxes"], case["im_id"], T, CLIP_MEAN, CLIP_STD)
    for v in case["ref_dense"] + case["ref_fused"]:
        v.setflags(write=False)
    return case


def test_crop_resize_pad_equals_aten_on_the_defect_sizes(aten_case):
    from gigapose_amd.crop import CropResizePad

    c, T = aten_case, aten_case["T"]
    images = np.ascontiguousarray(np.broadcast_to(c["image5"], (len(c["boxes"]),) + c["image5"].shape))
    out = CropResizePad(target_size=T)(_t(c["boxes"]), _t(images))
    got = out["images"].cpu().numpy()
    for d, box in enumerate(c["boxes"]):
        np.testing.assert_array_equal(got[d].view(np.uint32), c["ref_dense"][0][d].view(np.uint32), err_msg=f"box {box.tolist()} at {T}")
    crop_aten.assert_M(out["M"].cpu().numpy(), c["ref_dense"][1])


def test_preprocess_detections_equals_aten_on_the_defect_sizes(aten_case):
    from gigapose_amd.crop import DetectionPreprocessor

    c, T = aten_case, aten_case["T"]
    out = DetectionPreprocessor(target_size=T)(_t(c["rgb"]), _t(c["masks"]), _t(c["boxes"]), _t(c["im_id"]))
    img, mask, M = c["ref_fused"]
    got_img, got_mask = out["tar_img"].cpu().numpy(), out["tar_mask"].cpu().numpy()
    for d, box in enumerate(c["boxes"]):
        np.testing.assert_array_equal(got_mask[d], mask[d], err_msg=f"mask of box {box.tolist()} at {T}")
        np.testing.assert_array_equal(got_img[d].view(np.uint32), img[d].view(np.uint32), err_msg=f"box {box.tolist()} at {T}")
    crop_aten.assert_M(out["tar_M"].cpu().numpy(), M)


def test_refused_boxes_are_named_and_leave_the_other_items_untouched(aten_case):
    """The boxes ATen raises on (an empty slice, a scaled side of 0), planted among live ones: the public call names the bad
    item; the C entry flags one of them, writes none of them and writes every live item as if they were not there."""
    from gigapose_amd import _lib
    from gigapose_amd.crop import CropResizePad

    c, T = aten_case, aten_case["T"]
    H, W = crop_aten.GPU_FRAME
    live, refused = c["boxes"][:3], c["refused"]
    img3 = np.ascontiguousarray(np.broadcast_to(c["image5"], (3,) + c["image5"].shape))
    for box in refused:
        assert crop_aten.aten_crop_or_error(torch.from_numpy(c["image5"]), box, T)[2] is not None      # ATen raises as well
        with pytest.raises(ValueError, match="detection 1 has an empty / out-of-frame box"):
            CropResizePad(target_size=T)(_t(np.stack([live[0], box, live[1]])), _t(img3))
    boxes = np.concatenate([np.stack([l, r]) for l, r in zip(np.resize(live, (len(refused), 4)), refused)])   # live, bad, live, bad ...
    D, sentinel = len(boxes), -7.5
    images = _t(np.ascontiguousarray(np.broadcast_to(c["image5"], (D,) + c["image5"].shape)))
    out = torch.full((D, 5, T, T), sentinel, device=DEV)
    M = torch.full((D, 3, 3), sentinel, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    d_boxes = _t(boxes)
    _lib.call("gp_crop_resize_pad", _lib.ptr(images), _lib.ptr(d_boxes), _lib.i(D), _lib.i(5), _lib.i(H), _lib.i(W), _lib.i(T),
              _lib.ptr(out), _lib.ptr(M), _lib.ptr(err), _lib.stream_ptr())
    flag = int(err.item())
    assert flag >= 1 and (flag - 1) % 2 == 1, flag                       # one of the bad items (odd positions)
    assert bool((out[1::2] == sentinel).all()) and bool((M[1::2] == sentinel).all()), "a refused item was written"
    idx = [i % 3 for i in range(len(refused))]
    np.testing.assert_array_equal(out[0::2].cpu().numpy(), c["ref_dense"][0][idx])
    crop_aten.assert_M(M[0::2].cpu().numpy(), c["ref_dense"][1][idx])


def test_crop_kernel_matches_the_reference_golden_of_sizes(golden_dir):
    """crop_sizes.npz: the unmodified CropResizePad(target_size=56) on the same box list (oracle/make_goldens.py gen_crop_sizes)."""
    from gigapose_amd.crop import CropResizePad

    g = np.load(os.path.join(golden_dir, "crop_sizes.npz"))
    H, W = crop_aten.GPU_FRAME
    image = crop_aten.index_image(H, W)
    assert image.astype(np.float64).sum() + g["boxes"].sum() == float(g["input_checksum"])
    images = np.ascontiguousarray(np.broadcast_to(image, (len(g["boxes"]),) + image.shape))
    out = CropResizePad(target_size=56)(_t(g["boxes"]), _t(images))
    np.testing.assert_array_equal(out["images"].cpu().numpy().view(np.uint32), g["images"].view(np.uint32))
    crop_aten.assert_M(out["M"].cpu().numpy(), g["M"])


def test_empty_batch_and_bad_box():
    from gigapose_amd.crop import CropResizePad

    out = CropResizePad()(torch.zeros(0, 4, dtype=torch.int64, device=DEV), torch.zeros(0, 3, 32, 32, device=DEV))
    assert out["images"].shape == (0, 3, 224, 224)
    with pytest.raises(ValueError):
        CropResizePad()(torch.tensor([[4, 4, 20, 20], [9, 9, 9, 12]], device=DEV), torch.zeros(2, 3, 32, 32, device=DEV))
