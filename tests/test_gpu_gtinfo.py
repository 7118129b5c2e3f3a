"""GPU: libgigapose_gtinfo.so (gpg_classify, gpg_count_runs, gpg_write_runs) and gigapose_amd/gtinfo.py against the numpy restatement
of include/gigapose_gtinfo.h (gigapose_testing/gtinfo_ref.py, which tests/test_gtinfo_host.py holds to independent readings), bit
for bit: every comparison is equality of integers or of bytes.  The one floating-point step, (Dm - Dt) <= delta, is held at its edge
by the planted pixels.  Frames of at most 96 x 128 except the one case past a 32-bit offset."""
import functools

import numpy as np
import pytest
import torch

from gigapose_amd import evaluate, gtinfo, hypotheses, ingest, inout, render, verify
from gigapose_testing import gtinfo_cases as cases
from gigapose_testing import gtinfo_ref, raster_ref
from gigapose_testing import refine_cases as rc
from gigapose_testing.gpu_cases import DEV, assert_bits, five_pairs
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu
NAMES = ("cls", "info", "box", "status")


def device_classify(vis, origin, depth, frame, ray, ray_index, delta):
    return gtinfo.classify(_t(vis), origin, None if depth is None else _t(depth), None if depth is None else _t(np.asarray(frame, np.int32)), _t(ray),
                           _t(np.asarray(ray_index, np.int32)), delta)


def check_classify(what, args):
    want = gtinfo_ref.classify(*args)
    got = device_classify(*args)
    for name, g, w in zip(NAMES, got, want):
        assert_bits(g, w, f"{what}: {name}")
    return want


# ---------------------------------------------------------------------------------------------- 1. gpg_classify
FRAMES = ((1, 1), (37, 23), (65, 63), (96, 128))


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("margin", (0, 1, "odd"))
def test_classify_equals_the_restatement_on_planted_cases(H, W, margin):
    """Margin 0 (the canvas is the frame), 1.0 and an odd canvas: the 64 x 64 tiles' edges fall inside, on and outside the frame."""
    canvas, origin = cases.origins(H, W)[(0, 1, "odd").index(margin)]
    case = cases.planted_case(H, W, canvas, origin, seed=H)
    want = check_classify("planted", cases.call(case))
    P = len(case["expect"])
    assert want[1][:P, gtinfo_ref.PX_VISIB].tolist() == [e[1] for e in case["expect"]]          # the restatement reads the planted pixels as named
    assert want[1][P:, gtinfo_ref.PX_ALL].any() and not want[3].any()
    check_classify("planted, no depth", cases.call(case, depth=None))


def test_classify_does_not_depend_on_the_order_or_the_split_of_the_call():
    case = cases.planted_case(65, 63, *cases.origins(65, 63)[1], seed=3)
    vis, origin, depth, frame, ray, ray_index, delta = cases.call(case)
    want = gtinfo_ref.classify(vis, origin, depth, frame, ray, ray_index, delta)
    order = np.random.RandomState(2).permutation(len(vis))
    got = device_classify(vis[order], origin, depth, frame[order], ray, ray_index[order], delta)
    for name, g, w in zip(NAMES, got, want):
        assert_bits(g, w[order], f"permuted: {name}")
    half = len(vis) // 2
    for sl in (slice(0, half), slice(half, None)):
        got = device_classify(vis[sl], origin, depth, frame[sl], ray, ray_index[sl], delta)
        for name, g, w in zip(NAMES, got, want):
            assert_bits(g, w[sl], f"split: {name}")


def test_classify_marks_bad_pairs_between_good_ones():
    case = cases.planted_case(37, 23, *cases.origins(37, 23)[1], seed=5)
    vis, origin, depth, frame, ray, ray_index, delta = cases.call(case)
    frame, ray_index = frame.copy(), ray_index.copy()
    frame[1], ray_index[6], frame[9], ray_index[9], frame[-2], ray_index[-1] = len(depth), -1, -1, len(ray), 2 ** 31 - 1, -2 ** 31
    want = check_classify("bad pairs", (vis, origin, depth, frame, ray, ray_index, delta))
    assert want[3][[1, 6, 9]].tolist() == [gtinfo.BAD_FRAME, gtinfo.BAD_RAY, gtinfo.BAD_FRAME | gtinfo.BAD_RAY] and want[3][-1] == gtinfo.BAD_RAY
    assert (want[3] == 0).sum() == len(vis) - 5 and want[1][want[3] == 0].any()
    want = check_classify("bad pairs, no depth", (vis, origin, None, frame, ray, ray_index, delta))           # the frame is not read
    assert want[3][[1, 6, 9]].tolist() == [0, gtinfo.BAD_RAY, gtinfo.BAD_RAY]


@functools.lru_cache(maxsize=None)
def drawn_pairs(margin):
    """gpu_cases.five_pairs drawn by render.project + render.raster on the canvas of `margin` -> keys (5,Hc,Wc) u64, origin."""
    poses, frame_keys = five_pairs()
    if margin == 0:
        return frame_keys, (0, 0)
    v, f = rc.mesh("boxes")
    Hc, Wc, ox, oy = gtinfo.canvas(rc.H, rc.W, margin)
    K = np.asarray(rc.K, np.float64).copy()
    K[2], K[5] = K[2] + ox, K[5] + oy
    xy, vd = render.project(_t(v), _t(poses.astype(np.float32)), K, 1e-3)
    vis, clipped = render.raster(xy, vd, _t(f), Hc, Wc)
    assert not clipped.any().item()
    vis = vis.cpu().numpy().view(np.uint64)
    vis.setflags(write=False)
    return vis, (ox, oy)


@pytest.mark.parametrize("margin", (0, 1.0))
def test_classify_equals_the_restatement_on_rendered_keys(margin):
    vis, origin = drawn_pairs(margin)
    depth = np.stack([rc.sensor_depth("boxes", 0), rc.sensor_depth("boxes", 1)])
    ray = evaluate.ray_map(rc.K, rc.H, rc.W)[None]
    frame = np.asarray([0, 0, 0, 1, 1], np.int32)
    for delta in (15.0, 0.0, 1e9):
        want = check_classify(f"rendered, delta {delta}", (vis, origin, depth, frame, ray, np.zeros(5, np.int32), delta))
        assert (want[1][:, gtinfo_ref.PX_ALL] > 200).all() and (want[1][:, gtinfo_ref.PX_VALID] == want[1][:, gtinfo_ref.PX_FRAME]).all()
    assert (want[1][:, gtinfo_ref.PX_VISIB] == want[1][:, gtinfo_ref.PX_FRAME]).all()                     # delta 1e9 hides nothing
    if margin:                                                                                             # the frame window of the canvas is the frame-sized drawing here
        assert (vis[:, origin[1]:origin[1] + rc.H, origin[0]:origin[0] + rc.W] != raster_ref.EMPTY_KEY).sum() > 1000


def test_classify_takes_65535_instances_of_a_1_x_1_frame():
    N = 65535
    rs = np.random.RandomState(7)
    kinds = cases.planted_pixels()
    which = rs.randint(0, len(kinds), N)
    vis = np.asarray([k[1] for k in kinds], np.uint64)[which].reshape(N, 1, 1)
    depth = np.asarray([k[2] for k in kinds], np.float32).reshape(-1, 1, 1)
    ray = np.asarray([k[3] for k in kinds], np.float64).reshape(-1, 1, 1)
    every = np.arange(len(kinds), dtype=np.int32)                                                      # an instance's rows depend on its kind alone
    per_kind = gtinfo_ref.classify(np.asarray([k[1] for k in kinds], np.uint64).reshape(-1, 1, 1), (0, 0), depth, every, ray, every, cases.DELTA)
    assert per_kind[1][:, gtinfo_ref.PX_VISIB].tolist() == [k[5] for k in kinds]
    got = device_classify(vis, (0, 0), depth, which.astype(np.int32), ray, which.astype(np.int32), cases.DELTA)
    for name, g, w in zip(NAMES, got, per_kind):
        assert_bits(g, w[which], f"65535 instances: {name}")
    with pytest.raises(ValueError, match="65535"):
        gtinfo.classify(torch.zeros(N + 1, 1, 1, dtype=torch.int64, device=DEV), (0, 0), None, None, _t(ray), torch.zeros(N + 1, dtype=torch.int32, device=DEV), 1.0)


# ---------------------------------------------------------------------------------------------- 2. the run kernels
def scan_of(counts, offsets, H, W):
    """gpi_rle_scan of the lists -> cum on the device, and the error flag."""
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cum = ingest.RleDetectionPreprocessor().scan(counts, offsets, H, W, err)
    return cum, int(err.item())


def check_runs(what, cls, H, W):
    """Both bits of one cls (N,W,H): the lists equal the restatement's, cum is gpi_rle_scan of counts bit for bit with its error flag 0,
    and gpi_rle_decode of the lists is the dense bit."""
    cls_d = _t(cls)
    for which in (0, 1):
        counts, cum, offsets = gtinfo.encode_runs(cls_d, which)
        want = gtinfo_ref.encode_runs(cls, which)
        for name, g, w in zip(("counts", "cum", "offsets"), (counts, cum, offsets), want):
            assert_bits(g, w, f"{what}, which {which}: {name}")
        scanned, err = scan_of(counts, offsets, H, W)
        assert err == 0
        assert_bits(scanned, cum, f"{what}, which {which}: gpi_rle_scan of the counts")
        dense = ingest.RleDetectionPreprocessor().decode(counts, offsets, H, W)
        assert_bits(dense, ((cls >> which) & 1).transpose(0, 2, 1).astype(np.float32), f"{what}, which {which}: gpi_rle_decode")
    return want


def test_run_lists_around_the_multiples_of_the_chunk():
    C = gtinfo.pixels_per_workgroup()
    rs = np.random.RandomState(11)
    for HW in (C - 1, C, C + 1, 2 * C + 1):
        H, W = next((h, HW // h) for h in (64, 63, 17, 3, 1) if HW % h == 0)
        obj = np.stack([cases.chunk_edge_bits(HW, C, rs), np.zeros(HW, bool), np.ones(HW, bool), rs.uniform(size=HW) < 0.5])
        seen = obj & (rs.uniform(size=obj.shape) < 0.7)
        seen[0] = cases.chunk_edge_bits(HW, C, rs)
        cls = (obj * 1 + seen * 2).astype(np.uint8).reshape(len(obj), W, H)
        want = check_runs(f"H*W = {HW}", cls, H, W)
        planted = set(gtinfo_ref.transitions(((cls[0] >> 1) & 1).reshape(-1)).tolist())
        assert {p for p in (0, C - 1, C, C + 1, HW - 1) if p < HW} <= planted
        assert want[2][2] - want[2][1] == 1                                                               # all zeros: one run


def test_run_lists_of_the_checkerboard_and_the_small_masks():
    yy, xx = np.mgrid[0:65, 0:63]
    boards = np.stack([(yy + xx) % 2 == 0, (yy + xx) % 2 == 1])
    want = check_runs("checkerboard 65 x 63", cases.cls_of(boards, boards[::-1]), 65, 63)
    assert np.diff(want[2]).tolist() == [65 * 63, 65 * 63 + 1]                                            # which = 1: the boards swapped, pixel 0 set in the second
    for shape in {m.shape for _, m in cases.run_masks()}:
        masks = np.stack([m for _, m in cases.run_masks() if m.shape == shape])
        check_runs(f"small masks {shape}", cases.cls_of(masks, masks & np.roll(masks, 1, axis=2)), *shape)
    case = cases.planted_case(37, 23, *cases.origins(37, 23)[1], seed=9)
    cls = gtinfo_ref.classify(*cases.call(case))[0]
    check_runs("the cls of a planted case", cls, 37, 23)


def test_a_wrong_slice_reports_its_instance_and_writes_nothing():
    masks = np.stack([m for _, m in cases.run_masks() if m.shape == (5, 7)][:4])
    cls = cases.cls_of(masks)
    cls_d = _t(cls)
    counts, cum, offsets = gtinfo_ref.encode_runs(cls, 0)
    for bad, edits in (("one entry too many, the next one too few", ((slice(2, None), 1), (slice(3, None), -1))), ("two entries too many", ((slice(3, None), 2),)),
                       ("a negative start", ((slice(0, 1), -1),)), ("beyond the lists", ((slice(4, 5), 10 ** 6),))):
        off = offsets.copy()
        for where, by in edits:
            off[where] += by
        total = int(offsets[-1]) + 3
        runs, work = gtinfo.count_runs(cls_d, 0)
        assert_bits(runs, gtinfo_ref.count_runs(cls, 0), "runs")
        out = torch.full((total,), -7, dtype=torch.int32, device=DEV), torch.full((total,), -7, dtype=torch.int32, device=DEV)
        err = torch.full((1,), 99, dtype=torch.int32, device=DEV)
        gtinfo.write_runs(cls_d, 0, work, _t(off), out, err)
        want = np.full(total, -7, np.int32), np.full(total, -7, np.int32)
        want_err = gtinfo_ref.write_runs(cls, 0, off, *want)
        bad_ones = [n + 1 for n in range(4) if not (0 <= off[n] < off[n + 1] <= total) or off[n + 1] - off[n] != runs[n].item()]
        assert bad_ones and want_err in bad_ones and int(err.item()) in bad_ones, bad
        assert_bits(out[0], want[0], f"{bad}: counts against the sentinel fill")
        assert_bits(out[1], want[1], f"{bad}: cum against the sentinel fill")


# ---------------------------------------------------------------------------------------------- 3. past a 32-bit offset
def test_the_kernels_address_cls_and_keys_past_2_to_the_31_bytes():
    """513 instances of 2048 x 2048 (the canvas is the frame): the last instance's cls begins 2^31 bytes into the buffer, its keys 2^34.
    Only the first and the last instance are planted and compared; the others carry a frame index outside the stack and read nothing."""
    n, side = 513, 2048
    assert (n - 1) * side * side >= 2 ** 31
    need = n * side * side * 9 + (3 << 30)
    torch.cuda.empty_cache()                                                                              # what earlier tests left in the allocator's cache is free
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"the device has {free >> 30} GiB free, this case needs {need >> 30} GiB")
    rs = np.random.RandomState(13)
    planes = np.full((2, side, side), raster_ref.EMPTY_KEY, np.uint64)
    for p, (y, x) in zip(planes, ((0, 0), (1990, 1995))):
        p[y:y + 48, x:x + 48] = np.where(rs.uniform(size=(48, 48)) < 0.6, cases.key_of(300.0, 1), raster_ref.EMPTY_KEY)
    planes[1, -1, -1], planes[0, 0, 0] = cases.key_of(300.0, 2), cases.key_of(300.0, 2)                   # the very first and the very last pixel
    depth = rs.choice(np.asarray([0.0, 200.0, 400.0], np.float32), size=(1, side, side))
    ray = np.ones((1, side, side))
    want = gtinfo_ref.classify(planes, (0, 0), depth, [0, 0], ray, [0, 0], 15.0)
    vis = torch.empty(n, side, side, dtype=torch.int64, device=DEV)
    vis[0].copy_(_t(planes[0]))
    vis[-1].copy_(_t(planes[1]))
    frame = np.full(n, -1, np.int32)
    frame[0], frame[-1] = 0, 0
    cls, info, box, status = gtinfo.classify(vis, (0, 0), _t(depth), _t(frame), _t(ray), torch.zeros(n, dtype=torch.int32, device=DEV), 15.0)
    del vis
    ends = [0, n - 1]
    for name, g, w in zip(NAMES, (cls[ends], info[ends], box[ends], status[ends]), want):
        assert_bits(g, w, f"the first and the last instance: {name}")
    assert (status[1:-1] == gtinfo.BAD_FRAME).all().item() and not info[1:-1].any().item()
    for which in (0, 1):
        counts, cum, offsets = gtinfo.encode_runs(cls, which)
        w_counts, w_cum, w_off = gtinfo_ref.encode_runs(want[0], which)
        offsets = offsets.cpu().numpy()
        assert np.diff(offsets)[1:-1].tolist() == [1] * (n - 2) and np.diff(offsets)[ends].tolist() == np.diff(w_off).tolist()
        for g, w in ((counts, w_counts), (cum, w_cum)):
            g = g.cpu().numpy()
            assert_bits(np.concatenate([g[:offsets[1]], g[offsets[-2]:]]), w, f"the first and the last instance's lists, which {which}")
    del cls
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 4. GroundTruthInfo
@functools.lru_cache(maxsize=None)
def computed(margin=1.0):
    models, cameras, gts = cases.scene(names=cases.OCCLUDED_SCENE)
    gts = dict(gts)
    gts[(1, 2)] = [cases.ground_truth(cases.HALF_OUT), cases.ground_truth(cases.FRONT)]                   # a second image, a second group order
    cameras = dict(cameras)
    cameras[(1, 2)] = dict(cam_K=cases.K, depth=np.zeros((cases.H, cases.W), np.float32))
    got = gtinfo.GroundTruthInfo(models, cameras, delta=15.0, margin=margin).compute(gts, masks=True)
    want = gtinfo_ref.compute(models, cameras, gts, delta=15.0, margin=margin, masks=True)
    return models, cameras, gts, got, want


@pytest.mark.parametrize("margin", (1.0, 0.0))
def test_compute_equals_the_restatement_over_the_numpy_rasteriser(margin):
    _, _, gts, got, want = computed(margin)
    assert set(got) == set(want) == set(gts)
    flat = []
    for key in gts:
        assert len(got[key]) == len(want[key]) == len(gts[key])
        for g, w in zip(got[key], want[key]):
            for name in ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib", "mask", "mask_visib"):
                assert g[name] == w[name] and type(g[name]) is type(w[name]), (key, name, g[name], w[name])
            flat.append(w)
    fracts = [w["visib_fract"] for w in want[(1, 1)]]
    assert fracts[0] == fracts[1] == 1 and 0.1 < fracts[2] < 1 and fracts[3] < 0.1
    if margin:
        assert 0 < want[(1, 2)][0]["visib_fract"] < 1 and want[(1, 2)][0]["bbox_obj"][0] < 0
    # the device lists of all instances, in the order of .instances
    assert got.instances == [(1, 1, j) for j in range(4)] + [(1, 2, 0), (1, 2, 1)]
    for lists, name in ((got.masks.lists, "mask"), (got.masks_visib.lists, "mask_visib")):
        runs = [np.asarray(w[name]["counts"], np.int64) for w in flat]
        assert_bits(lists[0], np.concatenate([np.cumsum(r) for r in runs]).astype(np.int32), f"{name}: cum of all instances")
        assert_bits(lists[1], np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int32), f"{name}: offsets")


def test_the_device_lists_are_masks_for_the_verify_kernel():
    """verify.counts over the five drawn pairs with the visible masks of the scene: the device lists of compute() give the rows of
    the same masks packed on the host (hypotheses.pack_masks + scan_masks)."""
    models, cameras, gts, got, want = computed(1.0)
    poses, keys = five_pairs()
    segs = [w["mask_visib"] for key in gts for w in want[key]]
    det = np.asarray([0, 1, 2, 3, 5], np.int32)
    est = [dict(scene_id=1, im_id=1, obj_id=1) for _ in det]
    table = hypotheses.CameraTable("test", cameras, "required")
    runs, offsets, det_h, _, _ = hypotheses.pack_masks("test", est, [segs[d] for d in det], table)
    host_lists = hypotheses.scan_masks(runs, offsets, cases.H, cases.W, DEV)
    depth = _t(np.stack([rc.sensor_depth("boxes", 0)]))
    args = (_t(keys), depth, _t(np.zeros(5, np.int32)))
    box, tol = _t(rc.whole_frame(5)), _t(np.full(5, 6.0))
    rows_h, status_h = verify.counts(*args, host_lists, _t(det_h), box, tol)
    rows_d, status_d = verify.counts(*args, got.masks_visib.lists, _t(det), box, tol)
    assert not status_h.any().item() and not status_d.any().item()
    assert_bits(rows_d, rows_h, "gpv_counts with the device lists and with the host-packed lists")
    assert rows_h[:, 1:8:2].sum().item() > 0                                                              # the masks hold covered pixels
    # HypothesisVerifier.score: the device lists as `masks`, an estimate naming its mask by instance_id = the position in .instances,
    # against the same masks as dictionaries packed on the host; both kinds of mask, both boxes
    est = [dict(scene_id=1, im_id=1, obj_id=1, score=0.5, R=p[:3, :3], t=p[:3, 3], instance_id=int(d)) for p, d in zip(poses, det)]
    for name, on_device in (("mask_visib", got.masks_visib), ("mask", got.masks)):
        host = {i: w[name] for i, w in enumerate(w for key in gts for w in want[key])}
        for box in ("projected", "frame"):
            verifier = verify.HypothesisVerifier(models, cameras, box=box)
            a, b = verifier.score(est, on_device), verifier.score(est, host)
            assert_bits(np.stack([s["counts"] for s in a]), np.stack([s["counts"] for s in b]), f"score with the device lists of {name}, box {box}")
            for k in ("verify", "depth_fit", "iou", "verify_status"):
                assert [s[k] for s in a] == [s[k] for s in b], (name, box, k)
            assert all(s["verify_status"] == 0 for s in a) and any(s["iou"] > 0 for s in a)


def brute_force_counted(errors, threshold, valid):
    taken = []
    for row in errors:
        free = [g for g in range(len(row)) if g not in taken]
        if free:
            best = min(free, key=lambda g: (row[g], g))
            if row[best] < threshold:
                taken.append(best)
    return sum(1 for g in taken if valid[g])


def test_pose_scorer_with_min_visib_over_a_csv_gives_the_recalls_of_the_host_reading(tmp_path):
    models, cameras, gts, got, want = computed(1.0)
    gts = {(1, 1): gts[(1, 1)]}
    cameras = {(1, 1): cameras[(1, 1)]}
    # four estimates of image (1, 1): near the free, the front and the behind instance, and one ON the buried one
    names = cases.OCCLUDED_SCENE
    poses = np.stack([rc.moved(cases.POSES[n], [0, 1, 0], a, o) for n, a, o in zip(names, (1, 2, 0.5, 0), ((1, 0, 2), (0, 2, -3), (1, 1, 1), (0, 0, 0)))])
    np.savez(tmp_path / "0.npz", poses=poses.astype(np.float32), scores=np.asarray([0.6, 0.7, 0.8, 0.9], np.float32), object_id=np.ones(4, np.int64),
             scene_id=np.ones(4, np.int64), im_id=np.ones(4, np.int64), time=np.zeros(4), detection_time=np.zeros(4))
    top1 = inout.save_predictions_from_batched_predictions(str(tmp_path), "ycbv", "gigapose", "run", False)[0]
    targets = [dict(scene_id=1, im_id=1, obj_id=1, inst_count=4)]
    seen = gtinfo.with_visibility(gts, got)
    assert [g["visib_fract"] for g in seen[(1, 1)]] == [w["visib_fract"] for w in want[(1, 1)]]
    out = evaluate.PoseScorer(models, targets, seen, cameras, min_visib=0.1).score_csv(top1)
    plain = evaluate.PoseScorer(models, targets, gts, cameras)
    everyone = plain.score_csv(top1)
    assert out["targets"] == 3 and everyone["targets"] == 4
    # the host reading: the plain scorer's error tables, the restatement's fractions, brute-force matching
    (t, e), = plain.errors(evaluate.read_estimates(top1))
    valid = [w["visib_fract"] >= 0.1 for w in want[(1, 1)]]
    assert valid == [True, True, True, False]
    for i, th in enumerate(evaluate.CORRECT_THS):
        assert out["recall_mssd"][i] == brute_force_counted(e["mssd"].tolist(), th * cases.SCALE, valid) / 3
        assert out["recall_mspd"][i] == brute_force_counted(e["mspd"].tolist(), evaluate.MSPD_THS[i] * cases.W / 640.0, valid) / 3
        for k in range(len(evaluate.TAUS)):
            assert out["recall_vsd"][k][i] == brute_force_counted(e["vsd"][:, :, k].tolist(), th, valid) / 3
    assert out["recall_mssd"][-1] == 1.0 and everyone["recall_mssd"][-1] == 1.0                           # the three visible ones are found
    with pytest.raises(ValueError, match="visib_fract"):
        evaluate.PoseScorer(models, targets, gts, cameras, min_visib=0.1).score_csv(top1)
