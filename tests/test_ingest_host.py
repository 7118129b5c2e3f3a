"""CPU: the host half of gigapose_amd.ingest -- the run-length format against the reference encoder's golden
(tests/golden/rle_masks.npz, written by tools/make_rle_golden.py from the unmodified src/utils/mask.py:mask_to_rle), pack_rle's
checks, FrameIngest's box / label / infos handling -- and libgigapose_ingest.so against include/gigapose_ingest.h."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gigapose_amd import ingest
from gigapose_testing import synthetic as syn
from gigapose_testing.symbols import exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_masks(golden_dir):
    g = np.load(os.path.join(golden_dir, "rle_masks.npz"))
    out = []
    for i, name in enumerate(g["names"]):
        H, W = (int(v) for v in g["sizes"][i])
        bits = g["bits"][g["bit_offsets"][i]:g["bit_offsets"][i + 1]]
        mask = np.unpackbits(bits)[:H * W].reshape(H, W)
        out.append((str(name), mask, g["counts"][g["offsets"][i]:g["offsets"][i + 1]]))
    return int(g["seed"]), out


def decode_numpy(counts, H, W):
    """The parity rule of the format: pixel p = x*H + y lies in run j = #{i : cum[i] <= p}; its value is j & 1."""
    cum = np.cumsum(np.asarray(counts, np.int64))
    j = np.searchsorted(cum, np.arange(H * W), side="right")
    return (j & 1).astype(np.uint8).reshape(W, H).T


def test_golden_holds_the_cases_the_format_has(golden_dir):
    seed, masks = golden_masks(golden_dir)
    by_name = {n: (m, c) for n, m, c in masks}
    case = syn.detection_case(seed)
    assert len(masks) == 15
    for d in range(10):
        np.testing.assert_array_equal(by_name[f"ellipse_{d}"][0], case["masks"][d].astype(np.uint8))
        assert by_name[f"ellipse_{d}"][1][0] > 0          # none of the ten starts with a 1: the extra masks below do
    assert by_name["first_pixel_set"][0][0, 0] == 1 and by_name["first_pixel_set"][1][0] == 0
    assert by_name["all_zero"][1].tolist() == [480 * 640]
    assert by_name["all_one"][1].tolist() == [0, 480 * 640]
    hole = by_name["hole"][0]
    assert hole[250, 320] == 0 and hole[250, 150] == 1 and hole[250, 480] == 1 and hole[0, 0] == 0
    assert by_name["salt_and_pepper_37x53"][0].shape == (37, 53) and 0.3 < by_name["salt_and_pepper_37x53"][0].mean() < 0.7


def test_encoder_equals_the_reference_encoder_and_the_parity_rule_decodes(golden_dir):
    _, masks = golden_masks(golden_dir)
    for name, mask, ref_counts in masks:
        counts = ingest.mask_to_rle_counts(mask)
        assert counts.dtype == np.int32, name
        np.testing.assert_array_equal(counts, ref_counts, err_msg=name)
        assert int(counts.sum()) == mask.size
        np.testing.assert_array_equal(decode_numpy(ref_counts, *mask.shape), mask, err_msg=name)
        np.testing.assert_array_equal(ingest.mask_to_rle_counts(mask.astype(np.float32)), ref_counts, err_msg=name)   # f32 {0,1} masks too


def seg(mask):
    return {"counts": ingest.mask_to_rle_counts(mask).tolist(), "size": list(mask.shape)}


def test_pack_rle_offsets_and_dtype():
    rs = np.random.RandomState(3)
    masks = [(rs.rand(12, 17) < p).astype(np.uint8) for p in (0.5, 0.0, 1.0, 0.2)]
    counts, offsets = ingest.pack_rle([seg(m) for m in masks], 12, 17)
    assert counts.dtype == np.int32 and offsets.dtype == np.int32 and offsets.shape == (5,) and offsets[0] == 0
    assert offsets[-1] == len(counts)
    for d, m in enumerate(masks):
        np.testing.assert_array_equal(counts[offsets[d]:offsets[d + 1]], ingest.mask_to_rle_counts(m))
    counts, offsets = ingest.pack_rle([], 12, 17)
    assert counts.shape == (0,) and counts.dtype == np.int32 and offsets.tolist() == [0]


def test_pack_rle_rejections_name_the_detection():
    good = seg(np.eye(6, 8, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"detection 1.*size"):
        ingest.pack_rle([good, {"counts": good["counts"], "size": [8, 6]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 2.*compressed string counts.*out of scope"):
        ingest.pack_rle([good, good, {"counts": "PYn0", "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 0.*negative"):
        ingest.pack_rle([{"counts": [50, -2], "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 1.*sum to 47"):
        ingest.pack_rle([good, {"counts": [40, 7], "size": [6, 8]}], 6, 8)


def test_xywh_boxes_truncate_toward_zero_like_the_reference():
    """BoundingBox(b, "xywh"): [x, y, x+w, y+h] in float, THEN .long() -- the sum is truncated, not its terms."""
    b = np.array([[10.6, 20.7, 30.6, 40.7], [-0.5, -1.5, 20.25, 11.25], [3.0, 4.0, 5.0, 6.0], [7.9, 0.2, 0.3, 0.9]], np.float32)
    got = ingest.xywh_to_xyxy_long(b)
    assert got.dtype == np.int64
    assert got.tolist() == [[10, 20, 41, 61], [0, -1, 19, 9], [3, 4, 8, 10], [7, 0, 8, 1]]
    import torch

    t = torch.from_numpy(b)
    ref = torch.stack([t[:, 0], t[:, 1], t[:, 0] + t[:, 2], t[:, 1] + t[:, 3]], dim=1).long()
    assert got.tolist() == ref.tolist()
    assert ingest.xywh_to_xyxy_long([[10.6, 20.7, 30.6, 40.7]]).tolist() == [[10, 20, 41, 61]]


def _dets(rs, n, H, W, cats):
    out = []
    for i in range(n):
        m = np.zeros((H, W), np.uint8)
        m[2 + i:9 + i, 3:11] = 1
        out.append(dict(bbox=[3.5, 2.25 + i, 8.0, 7.5], category_id=int(cats[i]), score=float(rs.rand()), segmentation=seg(m), time=0.1))
    return out


def test_frame_ingest_host_half_labels_label_map_and_infos_rows():
    rs = np.random.RandomState(8)
    H, W = 20, 24
    infos = [dict(scene_id=2, view_id=7), dict(scene_id=2, view_id=9), dict(scene_id=5, view_id=1)]
    dets = [_dets(rs, 3, H, W, [8, 1, 12]), [], _dets(rs, 2, H, W, [5, 8])]
    counts, offsets, xyxy, im_id, frame = ingest.host_batch(infos, dets, H, W)
    assert len(frame) == 5 and offsets.shape == (6,) and xyxy.shape == (5, 4) and xyxy.dtype == np.int64
    assert im_id.dtype == np.int32 and im_id.tolist() == [0, 0, 0, 2, 2]
    assert frame.label.tolist() == ["8", "1", "12", "5", "8"]
    assert frame.scene_id.tolist() == [2, 2, 2, 5, 5] and frame.view_id.tolist() == [7, 7, 7, 1, 1]
    assert xyxy[1].tolist() == [3, 3, 11, 10]                  # [3.5, 3.25, 11.5, 10.75] truncated
    for d, det in enumerate(dets[0] + dets[2]):
        assert counts[offsets[d]:offsets[d + 1]].tolist() == det["segmentation"]["counts"]
    lmo = {1: 0, 5: 1, 8: 4, 12: 7}
    frame2 = ingest.host_batch(infos, dets, H, W, label_map=lmo)[4]
    assert frame2.label.tolist() == ["4", "0", "7", "1", "4"]
    empty = ingest.host_batch(infos[:1], [[]], H, W)
    assert len(empty[4]) == 0 and list(empty[4].columns)[:3] == ["label", "scene_id", "view_id"] and empty[2].shape == (0, 4)
    with pytest.raises(ValueError, match="detection 3"):
        dets[2][0]["segmentation"]["size"] = [W, H]
        ingest.host_batch(infos, dets, H, W)


# ---------------------------------------------------------------------------------------------- the library and its header
def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gigapose_ingest.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpi_[a-z0-9_]+)\s*\(", src)))


def test_ingest_library_exports_exactly_its_header_and_no_product_symbol():
    names = declared_symbols()
    assert names == ["gpi_abi_version", "gpi_last_error", "gpi_preprocess_detections_rle", "gpi_rle_decode", "gpi_rle_scan"]
    exported = exported_symbols(ingest.INGEST_LIB_PATH)
    assert [n for n in exported if n.startswith("gpi_")] == names
    assert not [n for n in exported if n.startswith("gp_")], "a hot-path symbol in the ingest library"
    lib = ingest.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gpi_abi_version() >= 1


def test_a_side_library_that_is_not_built_is_an_error_that_names_the_file_and_the_build_command():
    from gigapose_amd import _lib

    missing = _lib.SideLibrary("libgigapose_nowhere.so", "gpx")
    assert missing.path == os.path.join(os.path.dirname(ingest.INGEST_LIB_PATH), "libgigapose_nowhere.so")
    for use in (missing.lib, lambda: missing.call("gpx_abi_version")):
        with pytest.raises(_lib.GigaPoseHipError) as e:
            use()
        assert str(e.value) == (f"{missing.path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is deliberately no CPU / PyTorch fallback)")
    assert list(_lib.chunked(5, 2)) == [(0, 0, 2), (1, 2, 4), (2, 4, 5)] and list(_lib.chunked(0, 2)) == []
    assert _lib.first_bad([0, 3, 1], 10) == 12 and _lib.first_bad([0, 0], 10) is None


def test_the_two_existing_libraries_carry_no_ingest_symbol():
    from gigapose_amd import _lib

    for path in (_lib.LIB_PATH, _lib.PROBE_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert "gpi_" not in out, path


def test_ingest_argument_validation_needs_no_gpu():
    lib = ingest.lib()
    null = ctypes.c_void_p(0)
    assert lib.gpi_rle_scan(null, null, 10, 1, 480, 640, null, null, null) == -1
    assert b"gpi_rle_scan" in lib.gpi_last_error() and b"null" in lib.gpi_last_error()
    assert lib.gpi_rle_scan(null, null, 10, 1, 65536, 65536, null, null, null) == -1        # H*W >= 2^31
    assert b"bad sizes" in lib.gpi_last_error()
    assert lib.gpi_rle_decode(null, null, 10, 2, 0, 640, null, null) == -1
    assert b"gpi_rle_decode" in lib.gpi_last_error()
    assert lib.gpi_preprocess_detections_rle(null, null, null, 10, null, null, 1, 3, 480, 640, 5000, null, null, null, null, null,
                                             null, null) == -1
    assert b"gpi_preprocess_detections_rle" in lib.gpi_last_error()
    assert lib.gpi_rle_scan(null, null, 0, 0, 480, 640, null, null, null) == 0              # D = 0: nothing to do
