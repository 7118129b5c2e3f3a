"""GPU: frames + run-length masks -> crops (libgigapose_ingest.so, gigapose_amd/ingest.py).

The fused run-length kernel against the reference golden (tests/golden/crop.npz, written by the unmodified CropResizePad) and,
bit for bit, against the dense-mask kernel it restates (gp_preprocess_detections); both branches of its search (runs staged in
LDS / searched in global memory); the decoder and the scan alone against numpy; the validated-input error paths; and the whole
route FrameIngest -> GigaPose.test_step against a batch assembled from the dense kernel's outputs."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

import dropin_flow as df
from gigapose_testing import factory
from gigapose_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(a).to(DEV)


def encode(masks):
    from gigapose_amd.ingest import mask_to_rle_counts

    lists = [mask_to_rle_counts(m) for m in masks]
    offsets = np.concatenate(([0], np.cumsum([len(c) for c in lists]))).astype(np.int32)
    return np.concatenate(lists).astype(np.int32), offsets


def decode_numpy(counts, H, W):
    cum = np.cumsum(np.asarray(counts, np.int64))
    return (np.searchsorted(cum, np.arange(H * W), side="right") & 1).astype(np.float32).reshape(W, H).T


def both_routes(case, target=224):
    """(dense route, run-length route) on the same frames, boxes and frame ids."""
    from gigapose_amd.crop import DetectionPreprocessor
    from gigapose_amd.ingest import RleDetectionPreprocessor

    counts, offsets = encode(case["masks"])
    rgb, boxes, im_id = _t(case["rgb"]), _t(case["boxes"]), _t(case["im_id"])
    dense = DetectionPreprocessor(target_size=target)(rgb, _t(case["masks"]), boxes, im_id)
    rle = RleDetectionPreprocessor(target_size=target)(rgb, _t(counts), _t(offsets), boxes, im_id)
    return dense, rle, (counts, offsets)


def assert_same_bits(a, b):
    for key in ("tar_img", "tar_mask", "tar_M"):
        x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
        assert x.shape == y.shape and x.dtype == y.dtype == np.float32
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=key)


def check_scan_and_decode(counts, offsets, masks):
    """gpi_rle_scan's cum == np.cumsum per detection; gpi_rle_decode == the numpy decoder (== the masks that were encoded)."""
    from gigapose_amd.ingest import RleDetectionPreprocessor

    D, H, W = masks.shape
    pre = RleDetectionPreprocessor()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cum = pre.scan(_t(counts), _t(offsets), H, W, err).cpu().numpy()
    assert int(err.item()) == 0
    for d in range(D):
        a, b = offsets[d], offsets[d + 1]
        np.testing.assert_array_equal(cum[a:b], np.cumsum(counts[a:b]), err_msg=f"detection {d}")
    dec = pre.decode(_t(counts), _t(offsets), H, W).cpu().numpy()
    for d in range(D):
        np.testing.assert_array_equal(dec[d], decode_numpy(counts[offsets[d]:offsets[d + 1]], H, W), err_msg=f"detection {d}")
    np.testing.assert_array_equal(dec, (masks != 0).astype(np.float32))


def test_rle_route_matches_reference_golden(golden_dir):
    from gigapose_amd.ingest import RleDetectionPreprocessor

    g = np.load(os.path.join(golden_dir, "crop.npz"))
    case = syn.detection_case(seed=int(g["seed"]))
    counts, offsets = encode(case["masks"])
    out = RleDetectionPreprocessor()(_t(case["rgb"]), _t(counts), _t(offsets), _t(case["boxes"]), _t(case["im_id"]))
    np.testing.assert_array_equal(out["tar_mask"].cpu().numpy(), g["tar_mask"])
    np.testing.assert_array_equal(out["tar_img"].cpu().numpy().view(np.uint32), g["tar_img"].view(np.uint32))
    np.testing.assert_allclose(out["tar_M"].cpu().numpy(), g["M"], rtol=2e-7, atol=0)
    check_scan_and_decode(counts, offsets, case["masks"])


def ragged_case(seed, H, W, D):
    """detection_case with ragged masks (ellipse XOR 10 % noise) and the special lists planted: all zero, all one, pixel (0,0)
    set, and a detection whose box lies wholly outside its mask."""
    case = syn.detection_case(seed=seed, n_img=2, D=D, H=H, W=W)
    rs = np.random.RandomState(seed + 1000)
    masks = np.logical_xor(case["masks"] != 0, rs.rand(D, H, W) < 0.1).astype(np.float32)
    masks[3] = 0.0
    masks[4] = 1.0
    masks[5, :H // 3, :W // 4] = 1.0
    masks[6] = 0.0
    masks[6, :H // 8, :W // 8] = 1.0                                   # mask in the top-left corner ...
    case["boxes"][6] = (W // 2, H // 2, W // 2 + W // 5, H // 2 + H // 4)   # ... box in the lower right quarter
    case["masks"] = masks
    return case


@pytest.mark.parametrize("target", [224, 112])
@pytest.mark.parametrize("seed,H,W,D", [(5, 480, 640, 40), (6, 97, 131, 25), (7, 1080, 1920, 12)])
def test_rle_route_equals_dense_route_bit_for_bit(seed, H, W, D, target):
    case = ragged_case(seed, H, W, D)
    dense, rle, (counts, offsets) = both_routes(case, target)
    assert_same_bits(dense, rle)
    assert float(rle["tar_mask"][6].abs().max()) == 0.0               # box outside the mask: an empty crop mask
    if target == 224:
        check_scan_and_decode(counts, offsets, case["masks"])


@pytest.mark.parametrize("target", [224, 37])
def test_rle_route_and_frame_ingest_equal_the_dense_route_on_the_defect_sizes(target):
    """The box list of the crop tests against ATen (gigapose_testing/crop_aten.py: the long sides whose scale has two roundings,
    the doubled / kept extents on either side of ATen's kernel choice, clamped, identity and 2x boxes): the run-length kernel
    and FrameIngest around it write the dense kernel's bits -- which tests/test_gpu_crop.py holds to ATen at these boxes."""
    from gigapose_amd.crop import DetectionPreprocessor
    from gigapose_amd.ingest import FrameIngest, RleDetectionPreprocessor, mask_to_rle_counts
    from gigapose_testing import crop_aten

    case = crop_aten.gpu_case(target)
    H, W = crop_aten.GPU_FRAME
    dense, rle, (counts, offsets) = both_routes(case, target)
    assert_same_bits(dense, rle)
    boxes = case["boxes"]
    dets = [[dict(bbox=[int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])], category_id=1, score=0.5, time=0.05,
                  segmentation=dict(counts=mask_to_rle_counts(m).tolist(), size=[H, W])) for b, m in zip(boxes, case["masks"])]]
    batch = FrameIngest(target_size=target)(case["rgb"], np.eye(3, dtype=np.float32)[None], [dict(scene_id=1, view_id=1)], dets)
    for key in ("tar_img", "tar_mask", "tar_M"):
        assert torch.equal(getattr(batch, key), dense[key]), key
    # a refused box among them: both routes name it, in the same words
    bad = dict(case, boxes=np.concatenate([boxes[:2], case["refused"][-1:], boxes[2:4]]), masks=case["masks"][:5], im_id=case["im_id"][:5])
    c5, o5 = encode(bad["masks"])
    with pytest.raises(ValueError, match="detection 2 has an empty / out-of-frame box") as e_dense:
        DetectionPreprocessor(target_size=target)(_t(bad["rgb"]), _t(bad["masks"]), _t(bad["boxes"]), _t(bad["im_id"]))
    with pytest.raises(ValueError, match="detection 2 has an empty / out-of-frame box") as e_rle:
        RleDetectionPreprocessor(target_size=target)(_t(bad["rgb"]), _t(c5), _t(o5), _t(bad["boxes"]), _t(bad["im_id"]))
    assert str(e_dense.value).split(": ", 1)[1] == str(e_rle.value).split(": ", 1)[1]


def runs_in_span(counts, H, x0, x1):
    """List entries a block has to look at for the columns [x0, x1): prefix sums in (x0*H, x1*H - 1]."""
    cum = np.cumsum(counts.astype(np.int64))
    return int(np.searchsorted(cum, x1 * H - 1, side="right") - np.searchsorted(cum, x0 * H, side="right"))


def test_both_search_branches_equal_the_dense_route():
    """A full-frame box on a 50 % random mask: ~150 k runs, beyond ANY LDS budget (160 KB hold 40 k int32) -- every pixel searches
    global memory.  A small box on a smooth mask: a few hundred runs, staged in LDS.  The same two detections give the same bits
    alone (D = 1) and inside D = 40."""
    H, W, D = 480, 640, 40
    case = syn.detection_case(seed=21, n_img=2, D=D, H=H, W=W)
    rs = np.random.RandomState(22)
    big, small = 11, 17
    case["masks"][big] = (rs.rand(H, W) < 0.5).astype(np.float32)
    case["boxes"][big] = (0, 0, W, H)
    case["boxes"][small] = (300, 200, 360, 270)
    yy, xx = np.mgrid[0:H, 0:W]
    case["masks"][small] = ((((xx - 330) / 40.0) ** 2 + ((yy - 235) / 30.0) ** 2) <= 1.0).astype(np.float32)
    counts, offsets = encode(case["masks"])
    n_big = runs_in_span(counts[offsets[big]:offsets[big + 1]], H, 0, W)
    n_small = runs_in_span(counts[offsets[small]:offsets[small + 1]], H, 300, 360)
    assert n_big > 140000 and offsets[big + 1] - offsets[big] > 140000     # > 40960: cannot be staged, longer than one scan pass
    assert 0 < n_small <= 256
    dense, rle, _ = both_routes(case)
    assert_same_bits(dense, rle)
    check_scan_and_decode(counts, offsets, case["masks"])                  # incl. the 150 k-run list and lists of other lengths
    for d in (big, small):
        one = dict(rgb=case["rgb"], masks=case["masks"][d:d + 1], boxes=case["boxes"][d:d + 1], im_id=case["im_id"][d:d + 1])
        dense1, rle1, _ = both_routes(one)
        assert_same_bits(dense1, rle1)
        for key in ("tar_img", "tar_mask", "tar_M"):
            assert torch.equal(rle1[key][0], rle[key][d]), f"detection {d}: {key} differs between D = 1 and D = {D}"


def test_scan_and_decode_of_a_list_of_length_one():
    H, W = 37, 53
    masks = np.zeros((3, H, W), np.float32)
    masks[1] = 1.0
    masks[2, 5:9, 7:30] = 1.0
    counts, offsets = encode(masks)
    assert offsets.tolist()[:3] == [0, 1, 3] and counts[:3].tolist() == [H * W, 0, H * W]
    check_scan_and_decode(counts, offsets, masks)


def _raw_call(rgb, counts, offsets, boxes, im_id, H, W, T, sentinel):
    """The C-ABI directly, past the host checks: outputs pre-filled with `sentinel`; returns (scan flag, crop flag, outputs)."""
    from gigapose_amd import _lib, ingest
    from gigapose_amd.crop import CLIP_MEAN, CLIP_STD

    lib = ingest.lib()
    D, n_img = len(offsets) - 1, rgb.shape[0]
    d_counts, d_offsets = _t(counts), _t(offsets)
    cum = torch.zeros_like(d_counts)
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    tar_img = torch.full((D, 3, T, T), sentinel, device=DEV)
    tar_mask = torch.full((D, T, T), sentinel, device=DEV)
    M = torch.full((D, 3, 3), sentinel, device=DEV)
    mean, std = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)
    d_rgb, d_boxes, d_im = _t(rgb), _t(boxes), _t(im_id)
    rc = lib.gpi_rle_scan(_lib.ptr(d_counts), _lib.ptr(d_offsets), _lib.i(len(counts)), _lib.i(D), _lib.i(H), _lib.i(W), _lib.ptr(cum),
                          _lib.ptr(err[0:1]), _lib.stream_ptr())
    assert rc == 0
    rc = lib.gpi_preprocess_detections_rle(_lib.ptr(d_rgb), _lib.ptr(cum), _lib.ptr(d_offsets), _lib.i(len(counts)), _lib.ptr(d_boxes),
                                           _lib.ptr(d_im), _lib.i(n_img), _lib.i(D), _lib.i(H), _lib.i(W), _lib.i(T), mean, std,
                                           _lib.ptr(tar_img), _lib.ptr(tar_mask), _lib.ptr(M), _lib.ptr(err[1:2]), _lib.stream_ptr())
    assert rc == 0
    masks = torch.full((D, H, W), sentinel, device=DEV)
    rc = lib.gpi_rle_decode(_lib.ptr(cum), _lib.ptr(d_offsets), _lib.i(len(counts)), _lib.i(D), _lib.i(H), _lib.i(W), _lib.ptr(masks),
                            _lib.stream_ptr())
    assert rc == 0
    flags = err.tolist()
    return flags[0], flags[1], dict(tar_img=tar_img, tar_mask=tar_mask, tar_M=M), masks


def test_bad_run_list_sets_the_flag_and_leaves_its_outputs_untouched():
    """A list whose total is H*W - 1 (and, separately, one with a negative count): validated-input paths, nothing faults."""
    case = syn.detection_case(seed=31, n_img=2, D=6, H=120, W=160)
    H, W, T, sentinel = 120, 160, 224, -7.5
    counts, offsets = encode(case["masks"])
    good_dense, good_rle, _ = both_routes(case)
    for bad, edit in ((2, "short"), (4, "negative")):
        c = counts.copy()
        a = offsets[bad]
        assert offsets[bad + 1] - a >= 3
        if edit == "short":
            c[a + 1] -= 1                                   # total H*W - 1
        else:
            c[a + 1] += c[a + 2] + 1                        # a negative count, total still H*W
            c[a + 2] = -1
            assert c[a:offsets[bad + 1]].sum() == H * W
        scan_flag, crop_flag, out, masks = _raw_call(case["rgb"], c, offsets, case["boxes"], case["im_id"], H, W, T, sentinel)
        assert scan_flag == bad + 1 and crop_flag == bad + 1
        for key in ("tar_img", "tar_mask", "tar_M"):
            assert bool((out[key][bad] == sentinel).all()), f"{key} of the bad detection was written"
            keep = [d for d in range(6) if d != bad]
            assert torch.equal(out[key][keep], good_dense[key][keep]), key
        assert bool((masks[bad] == sentinel).all())
        assert torch.equal(masks[[d for d in range(6) if d != bad]], _t(case["masks"])[[d for d in range(6) if d != bad]])
    # the public interface raises, naming the detection (pack_rle would have caught it on the host; device-side lists skip pack_rle)
    from gigapose_amd.ingest import RleDetectionPreprocessor

    c = counts.copy()
    c[offsets[2] + 1] -= 1
    with pytest.raises(ValueError, match="detection 2 has a bad run-length list"):
        RleDetectionPreprocessor()(_t(case["rgb"]), _t(c), _t(offsets), _t(case["boxes"]), _t(case["im_id"]))
    # a slice that leaves the arrays: flagged by its offsets alone, nothing read or written through it
    o = offsets.copy()
    o[-1] += 5
    scan_flag, crop_flag, out, _ = _raw_call(case["rgb"], counts, o, case["boxes"], case["im_id"], H, W, T, sentinel)
    assert scan_flag == 6 and crop_flag == 6 and bool((out["tar_img"][5] == sentinel).all())
    assert torch.equal(out["tar_img"][:5], good_rle["tar_img"][:5])


def test_bad_box_empty_batch_and_cpu_tensors():
    from gigapose_amd import _lib
    from gigapose_amd.crop import DetectionPreprocessor
    from gigapose_amd.ingest import RleDetectionPreprocessor

    case = syn.detection_case(seed=33, n_img=1, D=4, H=64, W=80)
    case["boxes"][2] = (9, 9, 9, 12)                       # empty box
    counts, offsets = encode(case["masks"])
    with pytest.raises(ValueError, match="detection 2 has an empty / out-of-frame box") as dense_err:
        DetectionPreprocessor()(_t(case["rgb"]), _t(case["masks"]), _t(case["boxes"]), _t(case["im_id"]))
    with pytest.raises(ValueError, match="detection 2 has an empty / out-of-frame box") as rle_err:
        RleDetectionPreprocessor()(_t(case["rgb"]), _t(counts), _t(offsets), _t(case["boxes"]), _t(case["im_id"]))
    assert str(dense_err.value).split(": ", 1)[1] == str(rle_err.value).split(": ", 1)[1]
    out = RleDetectionPreprocessor()(_t(case["rgb"]), torch.zeros(0, dtype=torch.int32, device=DEV),
                                     torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, 4, dtype=torch.int64, device=DEV),
                                     torch.zeros(0, dtype=torch.int32, device=DEV))
    assert out["tar_img"].shape == (0, 3, 224, 224) and out["tar_mask"].shape == (0, 224, 224) and out["tar_M"].shape == (0, 3, 3)
    with pytest.raises(_lib.GigaPoseHipError):
        RleDetectionPreprocessor()(torch.from_numpy(case["rgb"]), counts, offsets, case["boxes"], case["im_id"])


# ------------------------------------------------------------------------------------------------ through the model
def cnos_frames(seed, sizes, n_obj, H=480, W=640):
    """Per frame: a u8 image, intrinsics and CNOS-style detection dicts (fractional xywh boxes, run-length masks)."""
    from gigapose_amd.ingest import mask_to_rle_counts

    rs = np.random.RandomState(seed)
    frames, Ks, infos, dets, dense = [], [], [], [], []
    for i, n in enumerate(sizes):
        case = syn.detection_case(seed=seed + 1 + i, n_img=1, D=max(n, 1), H=H, W=W)
        frames.append(case["rgb"][0])
        Ks.append(syn.crop_geometry(seed + 50 + i, 1)[0][0])
        infos.append(dict(scene_id=2, view_id=40 + i))
        cats = (np.arange(n) % n_obj) + 1
        rs.shuffle(cats)
        frame_dets, frame_dense = [], []
        for d in range(n):
            x0, y0, x1, y1 = (int(v) for v in case["boxes"][d])
            fx, fy = (0.0, 0.0) if x0 == 0 else tuple(rs.uniform(0.05, 0.95, 2))
            bbox = [x0 + fx, y0 + fy, (x1 - x0) + rs.uniform(0.0, 0.9), (y1 - y0) + rs.uniform(0.0, 0.9)]
            m = case["masks"][d]
            frame_dets.append(dict(bbox=bbox, category_id=int(cats[d]), score=float(rs.uniform(0.3, 0.9)), time=0.05,
                                   segmentation=dict(counts=mask_to_rle_counts(m).tolist(), size=[H, W])))
            frame_dense.append(m)
        dets.append(frame_dets)
        dense.append(np.stack(frame_dense) if frame_dense else np.zeros((0, H, W), np.float32))
    return np.stack(frames), np.stack(Ks), infos, dets, dense


def make_test_list(labels, view_id):
    from gigapose_amd.tensor_collection import PandasTensorCollection

    labels = np.asarray(labels, np.int64)
    objs = sorted(set(int(l) for l in labels))
    return PandasTensorCollection(infos=pd.DataFrame(dict(
        im_id=[view_id] * len(objs), scene_id=[2] * len(objs), obj_id=objs, inst_count=[int((labels == o).sum()) for o in objs],
        detection_time=[0.05] * len(objs))))


_MODEL = {}


def vits_model(log_dir, accumulate):
    if "m" not in _MODEL:
        model = factory.build_model("dinov2_vits14", k=5, device=DEV, seed=70, numerics="chain")
        syn.condition_ist(model.ist_net)
        _MODEL["m"] = model
    model = _MODEL["m"]
    model.set_numerics("chain")
    model.log_dir, model.accumulate_crops = str(log_dir), accumulate
    model.template_datasets = {"syn": factory.TemplateSet(2, 12, seed=90)}
    model.test_dataset_name = "syn"
    model.run_id = "r0"
    os.makedirs(os.path.join(model.log_dir, "predictions"), exist_ok=True)
    return model


def read_predictions(log_dir, n):
    pred_dir = os.path.join(str(log_dir), "predictions")
    files = []
    for i in range(n):
        with np.load(os.path.join(pred_dir, f"{i}.npz")) as z:
            files.append({k: z[k] for k in z.files})
    csvs = {f: pd.read_csv(os.path.join(pred_dir, f)) for f in sorted(os.listdir(pred_dir)) if f.endswith(".csv")}
    return files, csvs


@pytest.mark.parametrize("accumulate", [0, 64])
def test_frame_ingest_then_test_step_equals_the_dense_route(tmp_path, accumulate):
    """ViT-S, 2 objects x 12 templates, chain numerics; three frames with 5 / 9 / 0 detections.  Route A: FrameIngest -> test_step.
    Route B: a batch assembled by hand from DetectionPreprocessor's outputs (dense masks, boxes converted as the reference does)
    -> test_step.  The prediction files are equal in every field except `time`, the merged csv in every column except `time`."""
    from gigapose_amd.crop import DetectionPreprocessor
    from gigapose_amd.ingest import FrameIngest, xywh_to_xyxy_long
    from gigapose_amd.tensor_collection import PandasTensorCollection

    sizes = [5, 9, 0]
    frames, Ks, infos, dets, dense = cnos_frames(60, sizes, n_obj=2)
    test_lists = [make_test_list([d["category_id"] for d in dets[i]], infos[i]["view_id"]) for i in range(3)]
    ingest = FrameIngest(target_size=224)
    pinned = torch.from_numpy(frames).pin_memory()

    # route A
    model = vits_model(tmp_path / "rle", accumulate)
    batches_a = [ingest(pinned[i:i + 1], Ks[i:i + 1], infos[i:i + 1], dets[i:i + 1], test_list=test_lists[i]) for i in range(3)]
    assert [len(b) for b in batches_a] == sizes and batches_a[2].tar_img.shape == (0, 3, 224, 224)
    df.trainer_test(model, batches_a)
    a_files, a_csv = read_predictions(tmp_path / "rle", 3)

    # route B
    model = vits_model(tmp_path / "dense", accumulate)
    batches_b = []
    for i, n in enumerate(sizes):
        boxes = xywh_to_xyxy_long(np.asarray([d["bbox"] for d in dets[i]], np.float32).reshape(-1, 4))
        rows = pd.DataFrame(dict(label=[str(d["category_id"]) for d in dets[i]], scene_id=[2] * n, view_id=[infos[i]["view_id"]] * n))
        if n:
            out = DetectionPreprocessor()(_t(frames[i:i + 1]), _t(dense[i]), _t(boxes), torch.zeros(n, dtype=torch.int32, device=DEV))
            tar_K = _t(np.repeat(Ks[i:i + 1], n, axis=0))
        else:
            out = dict(tar_img=torch.empty(0, 3, 224, 224, device=DEV), tar_mask=torch.empty(0, 224, 224, device=DEV),
                       tar_M=torch.empty(0, 3, 3, device=DEV))
            tar_K = torch.empty(0, 3, 3, device=DEV)
        b = PandasTensorCollection(infos=rows, tar_img=out["tar_img"], tar_mask=out["tar_mask"], tar_K=tar_K, tar_M=out["tar_M"])
        b.test_list = test_lists[i]
        batches_b.append(b)
    for a, b in zip(batches_a, batches_b):     # the batches themselves: same tensors, same labels / ids, in detection order
        for key in ("tar_img", "tar_mask", "tar_K", "tar_M"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        for col in ("label", "scene_id", "view_id"):
            assert a.infos[col].tolist() == b.infos[col].tolist()
    df.trainer_test(model, batches_b)
    b_files, b_csv = read_predictions(tmp_path / "dense", 3)

    for i, n in enumerate(sizes):
        assert sorted(a_files[i]) == sorted(b_files[i]) and a_files[i]["poses"].shape == (n, 5, 4, 4)
        for key in a_files[i]:
            assert a_files[i][key].dtype == b_files[i][key].dtype and a_files[i][key].shape == b_files[i][key].shape
            if key != "time":
                assert a_files[i][key].tobytes() == b_files[i][key].tobytes(), f"image {i}: {key}"
    assert list(a_csv) == list(b_csv) and len(a_csv) == 2
    for name in a_csv:
        ca, cb = a_csv[name], b_csv[name]
        assert list(ca.columns) == list(cb.columns) and len(ca) == len(cb) and len(ca) > 0
        for col in ca.columns:
            if col != "time":
                assert ca[col].tolist() == cb[col].tolist(), f"{name}: column {col}"

    # all three frames in ONE call (n_img = 3): the per-frame batches, concatenated
    allb = ingest(pinned, Ks, infos, dets)
    assert len(allb) == 14 and allb.infos.view_id.tolist() == [40] * 5 + [41] * 9
    for key in ("tar_img", "tar_mask", "tar_K", "tar_M"):
        assert torch.equal(getattr(allb, key), torch.cat([getattr(b, key) for b in batches_a]))
