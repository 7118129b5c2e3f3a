"""CPU: the numpy restatement of the detection pre-processing stage (oracle/crop_numpy.py) against the goldens
written by the unmodified reference (CropResizePad + process_real arithmetic; oracle/make_goldens.py gen_crop, and
gen_crop_sizes: the long sides and extents at which the scale's two roundings and ATen's kernel choice show)."""
import os

import numpy as np
import pytest
import torch

from gigapose_testing import crop_aten
from gigapose_testing import synthetic as syn
from oracle import crop_numpy


def test_crop_restatement_matches_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "crop.npz"))
    case = syn.detection_case(seed=int(g["seed"]))
    chk = case["rgb"].astype(np.float64).sum() + case["masks"].sum() + case["boxes"].sum()
    assert chk == float(g["input_checksum"]), "synthetic inputs drifted from the ones the golden was made with"
    img, mask, M = crop_numpy.preprocess_detections(case["rgb"], case["masks"], case["boxes"], case["im_id"])
    np.testing.assert_array_equal(mask, g["tar_mask"])
    np.testing.assert_array_equal(img.view(np.uint32), g["tar_img"].view(np.uint32))   # bit-exact pixels
    crop_aten.assert_M(M, g["M"])                          # scale entries bit for bit, translations <= 1 ulp (matmul order)


def test_restatement_and_aten_chain_match_the_reference_golden_of_sizes(golden_dir):
    """crop_sizes.npz: the reference's CropResizePad(56) on the GPU tests' box list.  Both the restatement and the ATen
    chain that every sweep uses as its reference reproduce it bit for bit."""
    g = np.load(os.path.join(golden_dir, "crop_sizes.npz"))
    H, W = crop_aten.GPU_FRAME
    boxes, refused = crop_aten.gpu_boxes(56)
    image = crop_aten.index_image(H, W)
    assert image.astype(np.float64).sum() + boxes.sum() == float(g["input_checksum"]), "inputs drifted from the golden's"
    np.testing.assert_array_equal(boxes, g["boxes"])
    assert sum(crop_aten.is_scale_class(b, H, W, 56) and b[2] - b[0] != b[3] - b[1] for b in boxes) >= 12
    images = np.broadcast_to(image, (len(boxes),) + image.shape)
    for name, (img, M) in dict(restatement=crop_numpy.crop_resize_pad(images, boxes, 56), aten=crop_aten.aten_batch(image, boxes, 56)).items():
        np.testing.assert_array_equal(img.view(np.uint32), g["images"].view(np.uint32), err_msg=name)
        crop_aten.assert_M(M, g["M"], name)
    for b in refused:
        assert crop_aten.aten_crop_or_error(torch.from_numpy(image), b, 56)[2] is not None
        with pytest.raises(ValueError):
            crop_numpy.crop_geometry(b, H, W, 56)


def test_gpu_box_list_carries_both_defect_classes():
    H, W = crop_aten.GPU_FRAME
    boxes, refused = crop_aten.gpu_boxes(224)
    assert 56 <= len(boxes) <= 72 and len(refused) >= 4
    assert sum(crop_aten.is_scale_class(b, H, W, 224) and b[2] - b[0] != b[3] - b[1] for b in boxes) >= 12
    generic = [b for b in boxes if crop_aten.is_generic_kernel_class(b, H, W, 224)]
    assert sum(crop_aten.is_width_only_doubled(b, H, W, 224) for b in generic) >= 4
    assert sum(crop_aten.is_width_only_doubled((b[1], b[0], b[3], b[2]), W, H, 224) for b in generic) >= 4
    sums = {sum(crop_aten.first_resize(b, H, W, 224)[2:4]) for b in boxes}
    assert 128 in sums and 130 in sums                                     # both sides of ATen's kernel selection
    assert len(crop_aten.gpu_boxes(37)[1]) > len(refused)                  # narrow boxes scale to nothing at 37


def test_nearest_index_shortcuts_and_bounds():
    assert crop_numpy.nearest_index(224, 224).tolist() == list(range(224))
    assert crop_numpy.nearest_index(8, 4).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    # ATen's generic kernel (out_h + out_w > 128) has no shortcut: under a scale_factor just above 2 or 1 it floors
    s = float((np.float32(1.0) / np.float32(111)) * np.float32(224))                    # 2.018...
    assert crop_numpy.nearest_index(8, 4, s).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]       # the vectorized kernel: still dst >> 1
    assert crop_numpy.nearest_index(8, 4, s, shortcuts=False).tolist() == [0, 0, 0, 1, 1, 2, 2, 3]
    s = float((np.float32(1.0) / np.float32(222)) * np.float32(224))                    # 1.009...
    assert crop_numpy.nearest_index(5, 5, s).tolist() == [0, 1, 2, 3, 4]
    assert crop_numpy.nearest_index(5, 5, s, shortcuts=False).tolist() == [0, 0, 1, 2, 3]
    assert crop_numpy.nearest_index(8, 4, None, shortcuts=False).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]   # in / out = 0.5: the same
    idx = crop_numpy.nearest_index(224, 223)
    assert idx[0] == 0 and idx[-1] == 222 and (np.diff(idx) >= 0).all()
    idx = crop_numpy.nearest_index(int(np.floor(300 * (224 / 300))), 300, float(np.float32(224) / np.float32(300)))
    assert idx.max() <= 299 and (np.diff(idx) >= 0).all()


def test_bad_boxes_raise():
    for box in [(5, 5, 5, 9), (-3, 0, 10, 10), (700, 10, 720, 30)]:
        with pytest.raises(ValueError):
            crop_numpy.crop_geometry(box, 480, 640)
