"""CPU: the host half of gigapose_amd.onboard -- load_renders, the numpy alpha-box reference against PIL's getbbox(), the golden
tests/golden/onboard_templates.npz (written by tools/make_onboard_golden.py from PIL and the unmodified CropResizePad) against
the numpy restatement -- and libgigapose_onboard.so against include/gigapose_onboard.h."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from gigapose_amd import _lib, ingest, onboard
from gigapose_testing import renders
from gigapose_testing import synthetic as syn
from gigapose_testing.symbols import exported_symbols
from oracle import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the library and its header
def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gigapose_onboard.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpo_[a-z0-9_]+)\s*\(", src)))


def test_onboard_library_exports_exactly_its_header_and_no_symbol_of_the_other_libraries():
    names = declared_symbols()
    assert names == ["gpo_abi_version", "gpo_alpha_boxes", "gpo_crop_templates", "gpo_last_error"]
    exported = exported_symbols(onboard.ONBOARD_LIB_PATH)
    assert [n for n in exported if n.startswith("gpo_")] == names
    assert not [n for n in exported if n.startswith("gp_")], "a hot-path symbol in the onboard library"
    assert not [n for n in exported if n.startswith("gpi_")], "an ingest symbol in the onboard library"
    lib = onboard.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gpo_abi_version() >= 1


def test_the_three_existing_libraries_carry_no_onboard_symbol():
    for path in (_lib.LIB_PATH, _lib.PROBE_LIB_PATH, ingest.INGEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert "gpo_" not in out, path


def test_onboard_argument_validation_needs_no_gpu():
    lib = onboard.lib()
    null = ctypes.c_void_p(0)
    assert lib.gpo_alpha_boxes(null, 2, 480, 640, null, null, null) == -1
    assert b"gpo_alpha_boxes" in lib.gpo_last_error() and b"null" in lib.gpo_last_error()
    assert lib.gpo_alpha_boxes(null, 2, 65536, 65536, null, null, null) == -1                # H*W >= 2^31
    assert b"gpo_alpha_boxes" in lib.gpo_last_error() and b"bad sizes" in lib.gpo_last_error()
    assert lib.gpo_alpha_boxes(null, 65536, 480, 640, null, null, null) == -1                # N > 65535
    assert lib.gpo_alpha_boxes(null, 2, 0, 640, null, null, null) == -1
    assert lib.gpo_crop_templates(null, null, 2, 480, 640, 224, null, null, null, null, null, null, null) == -1
    assert b"gpo_crop_templates" in lib.gpo_last_error() and b"null" in lib.gpo_last_error()
    assert lib.gpo_crop_templates(null, null, 2, 480, 640, 5000, null, null, null, null, null, null, null) == -1
    assert b"gpo_crop_templates" in lib.gpo_last_error() and b"bad sizes" in lib.gpo_last_error()
    assert lib.gpo_alpha_boxes(null, 0, 480, 640, null, null, null) == 0                     # N = 0: nothing to do
    assert lib.gpo_crop_templates(null, null, 0, 480, 640, 224, null, null, null, null, null, null, null) == 0


def test_cpu_input_has_no_fallback():
    import torch

    rgba = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        onboard.alpha_boxes(rgba)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        onboard.TemplateOnboarder()(rgba)


# ---------------------------------------------------------------------------------------------- load_renders
def write_views(path, rgba, ids=None):
    from PIL import Image

    for i, view in zip(range(len(rgba)) if ids is None else ids, rgba):
        Image.fromarray(view).save(os.path.join(str(path), f"{i:06d}.png"))


def test_load_renders_round_trips_in_view_order(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rgba = renders.object_renders(7, 12, 24, 40)
    write_views(tmp_path, rgba[::-1], ids=range(11, -1, -1))        # written last view first: the order is by view id
    Image.fromarray(rgba[0, ..., 0]).save(os.path.join(str(tmp_path), "000003_depth.png"))   # the reference's depth file is not a view
    got = onboard.load_renders(tmp_path)
    assert got.dtype == np.uint8 and got.shape == (12, 24, 40, 4)
    np.testing.assert_array_equal(got, rgba)
    np.testing.assert_array_equal(onboard.load_renders(str(tmp_path), num_templates=5), rgba[:5])


def test_load_renders_rejections(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rgba = renders.object_renders(8, 4, 24, 40)
    rgb_dir, mixed_dir, gap_dir = (tmp_path / n for n in ("rgb", "mixed", "gap"))
    for d in (rgb_dir, mixed_dir, gap_dir):
        d.mkdir()
    write_views(rgb_dir, rgba)
    Image.fromarray(rgba[2, ..., :3]).save(os.path.join(str(rgb_dir), "000002.png"))
    with pytest.raises(ValueError, match=r"000002\.png.*RGB, not RGBA"):
        onboard.load_renders(rgb_dir)
    write_views(mixed_dir, rgba)
    Image.fromarray(rgba[1, :20]).save(os.path.join(str(mixed_dir), "000001.png"))
    with pytest.raises(ValueError, match=r"000001\.png is 40 x 20, view 0 is 40 x 24"):
        onboard.load_renders(mixed_dir)
    write_views(gap_dir, rgba[[0, 1, 3]], ids=[0, 1, 3])
    with pytest.raises(ValueError, match="view 2 is missing"):
        onboard.load_renders(gap_dir)
    assert onboard.load_renders(gap_dir, num_templates=2).shape == (2, 24, 40, 4)          # the views asked for are all there
    write_views(tmp_path, rgba)
    with pytest.raises(ValueError, match="view 4 is missing"):
        onboard.load_renders(tmp_path, num_templates=6)


# ---------------------------------------------------------------------------------------------- the generator and the golden
def generator_cases():
    names, big, boxes = renders.box_class_renders()
    yield "box classes", big, boxes
    yield "golden", renders.golden_renders(), np.asarray(renders.GOLDEN_BOXES, np.int64)
    yield "object", renders.object_renders(21, 6, 96, 128), None


def test_numpy_alpha_box_equals_pil_getbbox_on_every_generator_case():
    Image = pytest.importorskip("PIL.Image")
    for name, rgba, want in generator_cases():
        got = renders.alpha_boxes_numpy(rgba)
        if want is not None:
            np.testing.assert_array_equal(got, want, err_msg=name)
        H, W = rgba.shape[1:3]
        for n, view in enumerate(rgba):
            im = Image.fromarray(view)
            assert tuple(got[n]) == im.getbbox(), (name, n)
            assert (view[..., :3] > 0).all(), "the colour must be non-zero where alpha is 0"
            assert im.getbbox(alpha_only=False) == (0, 0, W, H), (name, n)      # an any-channel box is the full frame: wrong
    blank = np.zeros((1, 6, 9, 4), np.uint8)
    blank[..., :3] = 200
    assert Image.fromarray(blank[0]).getbbox() is None and renders.alpha_boxes_numpy(blank).tolist() == [[0, 0, 0, 0]]


def test_the_rim_of_a_render_carries_alpha_1_3_7_255():
    _, rgba, boxes = renders.box_class_renders()
    x0, y0, x1, y1 = boxes[10]                                        # 301 x 226: no two extreme pixels coincide
    a = rgba[10, ..., 3]
    rim = sorted(int(v.max()) for v in (a[:, x0], a[y0, :], a[:, x1 - 1], a[y1 - 1, :]))
    assert rim == [1, 3, 7, 255]
    assert len(np.unique(a)) == 256                                   # the mask has 256 levels


def test_golden_is_self_consistent_without_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "onboard_templates.npz"))
    rgba = renders.golden_renders(int(g["seed"]))
    assert str(g["input_checksum"]) == syn.checksum(rgba)
    assert len(rgba) <= 8 and os.path.getsize(os.path.join(golden_dir, "onboard_templates.npz")) < 1 << 20
    rgb, mask, M, boxes = renders.prepare_numpy(rgba)
    np.testing.assert_array_equal(boxes, g["boxes"])
    np.testing.assert_array_equal(boxes, np.asarray(renders.GOLDEN_BOXES))
    for name, got in (("rgb", rgb), ("mask", mask), ("M", M)):
        assert got.dtype == g[name].dtype == np.float32 and got.shape == g[name].shape, name
        np.testing.assert_array_equal(got.view(np.uint32), g[name].view(np.uint32), err_msg=name)
    assert len(np.unique(g["mask"])) > 200                            # not binarised


@pytest.mark.reference
@pytest.mark.skipif(not ref_shim.available(), reason="the reference tree is not here")
def test_golden_is_what_the_tool_writes_from_the_reference(golden_dir):
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_onboard_golden", os.path.join(ROOT, "tools", "make_onboard_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = np.load(os.path.join(golden_dir, "onboard_templates.npz"))
    ref = tool.reference_templates(renders.golden_renders(int(g["seed"])))
    np.testing.assert_array_equal(ref["boxes"], g["boxes"])
    for name in ("rgb", "mask", "M"):
        np.testing.assert_array_equal(ref[name].view(np.uint32), g[name].view(np.uint32), err_msg=name)
