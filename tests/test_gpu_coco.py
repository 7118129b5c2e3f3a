"""GPU: libgigapose_coco.so (gpc_fg_scan, gpc_mask_inter, gpc_box_inter, gpc_match, gpc_sup_bits) and gigapose_amd/detections.py
against the restatement of include/gigapose_coco.h (gigapose_testing/coco_ref.py, which tests/test_coco_host.py holds to dense
masks, pixel sets and Fractions), BIT FOR BIT: every comparison is equality of integers.  Then whole scores: ground truths of
GroundTruthInfo, detections made from their masks or labelled by ProposalLabeller on a randomly initialised ViT-S/14 -- which
proves plumbing, not accuracy: no checkpoint is available.

With a wrong variant of coco_ref standing in for the kernels these tests fail: even_runs, search_one_short ->
test_foreground_and_intersections_equal_the_restatement; strict_threshold, first_on_tie, no_ignore_preference, rematch ->
test_match_decides_the_planted_groups_as_worked_by_hand; no_envelope, float_recall are host arithmetic (tests/test_coco_host.py)."""
import functools
import os

import numpy as np
import pytest
import torch

from gigapose_amd import detections, gtinfo, proposals
from gigapose_amd.ingest import mask_to_rle_counts
from gigapose_testing import coco_cases as cases
from gigapose_testing import coco_ref as ref
from gigapose_testing import gtinfo_cases, label_ref
from gigapose_testing import synthetic as syn
from gigapose_testing.gpu_cases import DEV, K_SMALL, ZNEAR, assert_bits, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. gpc_fg_scan, gpc_mask_inter
@functools.lru_cache(maxsize=None)
def frame_case(H, W):
    """The lists of a frame, their restated prefix sums and the restated intersections of every pair, computed once."""
    names, lists = cases.frame_lists(H, W)
    cum, offsets = cases.pack_cum(lists)
    fg, area, status = ref.fg_scan(cum, offsets, H * W)
    a, b = cases.every_pair(len(lists))
    inter, pstatus = ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), H * W, a, b)
    assert not status.any() and not pstatus.any()
    for arr in (cum, offsets, fg, area, a, b, inter):
        arr.setflags(write=False)
    return dict(names=names, lists=lists, cum=cum, offsets=offsets, fg=fg, area=area, a=a, b=b, inter=inter, n=len(lists), HW=H * W)


def device_foreground(c):
    return detections.foreground((_t(c["cum"]), _t(c["offsets"])), c["HW"])


@pytest.mark.parametrize("H,W", cases.FRAMES)
def test_foreground_and_intersections_equal_the_restatement(H, W):
    """Every pair of: empty, full, pixel 0, the last pixel, runs that begin where another mask's end, random masks, lists of 1 .. 2049
    runs, and the complement of each."""
    c = frame_case(H, W)
    fg = device_foreground(c)
    assert_bits(fg.status, np.zeros(c["n"], np.int32), "status") or assert_bits(fg.area, c["area"], "area") or assert_bits(fg.fg, c["fg"], "fg")
    inter, status = detections.mask_intersections(fg, fg, _t(c["a"]), _t(c["b"]))
    assert_bits(status, np.zeros(c["n"] ** 2, np.int32), "pair status") or assert_bits(inter, c["inter"], "inter")
    m = c["inter"].reshape(c["n"], c["n"])
    half = c["n"] // 2
    assert (m == m.T).all() and (np.diag(m) == c["area"]).all()                                    # inter(a, b) == inter(b, a); A with A
    assert not m[np.arange(half), np.arange(half) + half].any()                                    # A with its complement
    assert (c["area"][:half] + c["area"][half:] == H * W).all()
    if H * W >= 8:
        assert sorted({len(x) for x in c["lists"]} & set(cases.RUN_COUNTS)) == list(cases.RUN_COUNTS)


def test_the_lists_of_the_ingest_scan_are_taken_as_they_are_and_equal_dense_masks_on_the_device():
    H, W = 48, 64
    c = frame_case(H, W)
    counts = np.concatenate(c["lists"]).astype(np.int32)
    cum, offsets, check = proposals.scan_lists("test", counts, c["offsets"], H, W, DEV)
    check()
    assert_bits(cum, c["cum"], "gpi_rle_scan's cum")
    fg = detections.foreground((cum, offsets), H * W)
    dense = torch.from_numpy(np.stack([cases.decode(x, H * W) for x in c["lists"]])).to(DEV)
    want = (dense[:, None, :] & dense[None, :, :]).sum(dim=2).reshape(-1)
    inter, _ = detections.mask_intersections(fg, fg, _t(c["a"]), _t(c["b"]))
    assert torch.equal(inter, want) and torch.equal(fg.area, dense.sum(dim=1))


def test_pairs_permuted_split_over_calls_and_counts_of_0_and_65535(monkeypatch):
    c = frame_case(1, 37)
    fg = device_foreground(c)
    rs = np.random.RandomState(8)
    pick = rs.randint(0, c["n"] ** 2, 65535)
    inter, status = detections.mask_intersections(fg, fg, _t(c["a"][pick]), _t(c["b"][pick]))
    assert_bits(inter, c["inter"][pick], "65535 pairs") or assert_bits(status, np.zeros(65535, np.int32), "status")
    inter, status = detections.mask_intersections(fg, fg, _t(c["a"][:0]), _t(c["b"][:0]))
    assert inter.shape == (0,) and status.shape == (0,)
    monkeypatch.setattr(detections, "MAX_ITEMS_PER_CALL", 7)                                       # 7 pairs, and 7 masks, per call
    inter, _ = detections.mask_intersections(fg, fg, _t(c["a"][pick[:100]]), _t(c["b"][pick[:100]]))
    assert_bits(inter, c["inter"][pick[:100]], "split over 15 calls")
    again = device_foreground(c)
    assert_bits(again.fg, c["fg"], "fg in chunks of 7 masks") or assert_bits(again.area, c["area"], "area in chunks")


def test_bad_masks_and_pairs_out_of_range_are_flagged_and_leave_their_neighbours_alone():
    H, W = 48, 64
    c = frame_case(H, W)
    cum, offsets = c["cum"].copy(), c["offsets"]
    bad = [3, 11]
    cum[offsets[bad[0] + 1] - 1] = -1                                                              # what a failed scan leaves
    cum[offsets[bad[1] + 1] - 1] = 37                                                              # the total of another frame
    sentinel = np.full(len(cum), 77, np.int32)
    want_fg, want_area, want_status = ref.fg_scan(cum, offsets, H * W, sentinel)
    assert want_status.nonzero()[0].tolist() == bad
    cum_d, off_d, fg_d = _t(cum), _t(offsets), _t(sentinel)
    area_d, status_d = torch.full((c["n"],), -1, dtype=torch.int64, device=DEV), torch.full((c["n"],), -1, dtype=torch.int32, device=DEV)
    L = detections._lib
    detections._call("gpc_fg_scan", L.ptr(cum_d), L.ptr(off_d), L.i(len(cum)), L.i(c["n"]), L.i(H * W), L.ptr(fg_d), L.ptr(area_d), L.ptr(status_d),
                     L.stream_ptr())
    assert_bits(fg_d, want_fg, "fg: a bad mask's part is not written") or assert_bits(area_d, want_area, "area") or assert_bits(status_d, want_status, "status")
    fg = detections.Foreground(cum_d, off_d, fg_d, area_d, status_d, H * W)
    a = np.asarray([0, 3, 1, -1, 2, c["n"], 5, 11, 6, 2 ** 31 - 1, 7, -2 ** 31], np.int32)
    b = np.asarray([1, 1, 11, 2, 3, 4, c["n"], 3, 7, 0, 8, 0], np.int32)
    want = ref.mask_inter((cum, offsets, want_fg), (cum, offsets, want_fg), H * W, a, b)
    assert want[1].tolist() == [0, 2, 2, 1, 2, 1, 1, 2, 0, 1, 0, 1]
    got = detections.mask_intersections(fg, fg, _t(a), _t(b))
    assert_bits(got[0], want[0], "inter") or assert_bits(got[1], want[1], "status")
    other = detections.Foreground(cum_d, off_d, fg_d, area_d, status_d, 37)                        # every mask is bad on another frame
    assert (detections.mask_intersections(other, other, _t(a[:1]), _t(b[:1]))[1] == ref.PAIR_MASK).all()


def test_box_intersections_equal_the_restatement():
    rs = np.random.RandomState(21)
    box_a = rs.randint(-20, 60, (40, 4)).astype(np.int32)
    box_b = np.concatenate([rs.randint(-20, 60, (30, 4)), [(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (0, 0, 2 ** 22, 5)]]).astype(np.int32)
    a = np.concatenate([rs.randint(0, 40, 300), [40, -1, 3]]).astype(np.int32)
    b = np.concatenate([rs.randint(0, 32, 300), [0, 0, 32]]).astype(np.int32)
    want = ref.box_inter(box_a, box_b, a, b)
    assert want[3][-3:].tolist() == [ref.PAIR_RANGE] * 3 and not want[3][:-3].any()
    got = detections.box_intersections(_t(box_a), _t(box_b), _t(a), _t(b))
    for name, g, w in zip(("inter", "area_a", "area_b", "status"), got, want):
        assert_bits(g, w, name)


# ---------------------------------------------------------------------------------------------- 2. gpc_match
def device_match(case, thresholds=cases.THRESHOLDS, den=cases.THR_DEN):
    return detections.match(*(_t(a) for a in cases.match_args(case)), thresholds, den)


def check_match(what, case, thresholds=cases.THRESHOLDS):
    want = ref.match(*cases.match_args(case), list(thresholds), cases.THR_DEN)
    got = device_match(case, thresholds)
    for name, g, w in zip(("dt_match", "dt_ignore", "status"), got, want):
        assert_bits(g, w, f"{what}: {name}")
    return want


def test_match_decides_the_planted_groups_as_worked_by_hand():
    planted = cases.planted_groups()
    case = cases.assemble([g[1:5] for g in planted])
    want = check_match("planted", case)
    assert not want[2].any()
    for q, (name, _, _, _, _, expect) in enumerate(planted):
        d0, d1 = case["det_off"][q:q + 2]
        assert want[0][0, d0:d1].tolist() == expect, name                                          # at 10 / 20
    check_match("planted, one threshold", case, (10,))


def test_match_equals_the_restatement_at_every_size_and_with_the_groups_permuted():
    """G = 0, 1, 63, 64, 65, 130 by D = 0, 1, 100, 101, small integers: equal IoUs as unequal fractions are common."""
    groups = cases.size_groups()
    case = cases.assemble(groups)
    want = check_match("sizes", case)
    assert not want[2].any() and (want[0] >= 0).any() and want[1].any()
    order = np.random.RandomState(5).permutation(len(groups))
    permuted = cases.assemble([groups[q] for q in order])
    got = device_match(permuted)
    for q_new, q in enumerate(order):
        (d0, d1), (e0, e1) = case["det_off"][q:q + 2], permuted["det_off"][q_new:q_new + 2]
        assert_bits(got[0][:, e0:e1], want[0][:, d0:d1], f"group {q} moved: dt_match")
        assert_bits(got[1][:, e0:e1], want[1][:, d0:d1], f"group {q} moved: dt_ignore")
    check_match("sizes, one threshold", case, (15,))


def test_match_flags_a_badly_ordered_group_and_a_group_that_leaves_the_arrays():
    good = ([[5]], [5], [5], [0])
    case = cases.assemble([good, ([[5, 5], [5, 5]], [5, 5], [5, 5], [1, 0]), good, good, good])
    case["pair_off"][3] = 99
    want = ref.match(*cases.match_args(case), [10, 12], 20, dt_match=np.full((2, 6), 7, np.int32), dt_ignore=np.full((2, 6), 7, np.uint8))
    assert want[2].tolist() == [0, ref.GROUP_ORDER, 0, ref.GROUP_RANGE, 0] and want[0][0].tolist() == [0, -1, -1, 0, 7, 0]
    args = [_t(a) for a in cases.match_args(case)]
    thr = _t(np.asarray([10, 12], np.int32))
    dt_match = torch.full((2, 6), 7, dtype=torch.int32, device=DEV)
    dt_ignore = torch.full((2, 6), 7, dtype=torch.uint8, device=DEV)
    status = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    L = detections._lib
    detections._call("gpc_match", L.ptr(args[0]), L.ptr(args[1]), L.ptr(args[2]), L.i(5), L.ptr(args[3]), L.i(len(case["inter"])), L.ptr(args[4]), L.i(6),
                     L.ptr(args[5]), L.ptr(args[6]), L.i(len(case["area_gt"])), L.ptr(thr), L.i(2), L.i(20), L.ptr(dt_match), L.ptr(dt_ignore), L.ptr(status),
                     L.stream_ptr())
    for name, g, w in zip(("dt_match", "dt_ignore", "status"), (dt_match, dt_ignore, status), want):
        assert_bits(g, w, name)


def test_match_takes_65535_groups_of_one_pair():
    rs = np.random.RandomState(31)
    Q = 65535
    area = rs.randint(1, 9, (2, Q)).astype(np.int64)
    inter = np.minimum(rs.randint(0, 9, Q), area.min(axis=0)).astype(np.int64)
    off = np.arange(Q + 1, dtype=np.int32)
    case = dict(det_off=off, gt_off=off, pair_off=off[:-1].copy(), inter=inter, area_det=area[0].copy(), area_gt=area[1].copy(),
                gt_ignore=(rs.uniform(size=Q) < 0.3).astype(np.uint8))
    union = area[0] + area[1] - inter
    hit = inter * 20 >= 10 * union                                                                 # one pair: the rule in one line
    got = device_match(case, (10,))
    assert_bits(got[0], np.where(hit, 0, -1).astype(np.int32)[None], "dt_match")
    assert_bits(got[1], (hit & (case["gt_ignore"] != 0)).astype(np.uint8)[None], "dt_ignore")
    assert not got[2].any().item() and 0 < hit.sum() < Q


# ---------------------------------------------------------------------------------------------- 3. gpc_sup_bits, mask_nms
def box_masks(P, H=64, W=64, seed=0):
    """P boxes inside an H x W frame and the run lists of the masks they fill: the box IoU and the mask IoU are the same fraction."""
    rs = np.random.RandomState(4000 + seed + P)
    x0, y0 = rs.randint(0, W - 8, P), rs.randint(0, H - 8, P)
    box = np.stack([x0, y0, x0 + rs.randint(1, 9, P), y0 + rs.randint(1, 9, P)], axis=1).astype(np.int32)
    if P > 2:
        box[2] = box[0]                                                                            # a duplicate, and a box inside another
        box[1] = (box[0, 0], box[0, 1], box[0, 2], max(box[0, 1] + 1, box[0, 3] - 1))
    lists = []
    for b in box:
        m = np.zeros((H, W), bool)
        m[b[1]:b[3], b[0]:b[2]] = True
        lists.append(mask_to_rle_counts(m))
    return box, lists


@pytest.mark.parametrize("P", (1, 64, 65, 2048))
def test_mask_nms_equals_the_restatement_and_the_box_nms_on_filled_boxes(P):
    H = W = 64
    box, lists = box_masks(P)
    cum, offsets = cases.pack_cum(lists)
    fg = detections.foreground((_t(cum), _t(offsets)), H * W)
    order = np.random.RandomState(P).permutation(P)
    b = box[order].astype(np.int64)
    iw = np.maximum(0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    ih = np.maximum(0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter, area = iw * ih, (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert_bits(fg.area, area[np.argsort(order)], "the masks' areas are the boxes'")
    for num, den in ((1, 4), (0, 1), (1, 1), (30000, 65536)):
        want_sup = ref.sup_bits(inter, area, num, den)
        got_sup = detections.sup_bits(_t(inter), _t(area), num, den)
        assert_bits(got_sup.cpu().numpy().view(np.uint64), want_sup, f"sup at {num}/{den}")
        if P <= 65:
            assert_bits(got_sup.cpu().numpy().view(np.uint64), label_ref.nms_matrix(box[order], None, num, den, False), f"the box NMS's matrix at {num}/{den}")
        want = label_ref.nms_keep(want_sup, P)
        keep = detections.mask_nms(fg, _t(order), num, den)
        assert_bits(keep, want, f"keep at {num}/{den}")
        assert_bits(proposals.nms(_t(box[order]), None, num, den), want, f"the box NMS at {num}/{den}")
        if P <= 65:
            assert_bits(keep, ref.mask_nms(cum, offsets, H * W, order, num, den), f"the restated mask NMS at {num}/{den}")
    if P > 2:
        assert want.sum() < P


def test_mask_nms_per_label_and_its_refusals():
    box, lists = box_masks(65)
    cum, offsets = cases.pack_cum(lists)
    fg = detections.foreground((_t(cum), _t(offsets)), 64 * 64)
    label = (np.arange(65) % 3).astype(np.int32)
    order = np.arange(65)
    want = label_ref.nms(box, label, 1, 4, True)
    assert_bits(detections.mask_nms(fg, _t(order), 1, 4, label=_t(label)), want, "per label") or assert_bits(proposals.nms(_t(box), _t(label), 1, 4, True), want, "boxes")
    with pytest.raises(ValueError, match="outside the set or is a bad list"):
        detections.mask_nms(fg, _t(np.asarray([0, 65])), 1, 4)
    assert detections.mask_nms(fg, _t(order[:0]), 1, 4).shape == (0,)


# ---------------------------------------------------------------------------------------------- 4. whole scores
@functools.lru_cache(maxsize=None)
def small_scene():
    """gtinfo_cases' scene of four ground truths of one object, one of them less than 10 % visible."""
    models, cameras, gts = gtinfo_cases.scene(names=gtinfo_cases.OCCLUDED_SCENE)
    table = gtinfo.GroundTruthInfo(models, cameras, delta=15.0, margin=1.0).compute(gts, masks=True)
    fracts = [r["visib_fract"] for r in table[(1, 1)]]
    assert fracts[3] < 0.1 < min(fracts[:3])
    return gts, table


def same_scores(got, want):
    for name in ("AP", "AP50", "AP75", "AR", "per_category"):
        assert got[name] == want[name], (name, got[name], want[name])
    assert got["cells"] == {k: v[:2] for k, v in want["cells"].items()}


@pytest.mark.parametrize("iou_type", ("segm", "bbox"))
@pytest.mark.parametrize("gt_mask", ("mask_visib", "mask"))
def test_the_ground_truths_submitted_as_detections_score_one(iou_type, gt_mask):
    gts, table = small_scene()
    H, W = gtinfo_cases.H, gtinfo_cases.W
    box = "bbox_visib" if gt_mask == "mask_visib" else "bbox_obj"
    rows = table[(1, 1)]
    dets = {(1, 1): [cases.detection(r[gt_mask]["counts"], H, W, 1, 0.9 - 0.1 * n, r[box]) for n, r in enumerate(rows)]}
    for source in (table, {k: list(v) for k, v in table.items()}):                                 # the device lists, and the host dictionaries
        scorer = detections.DetectionScorer(source, iou_type=iou_type, gt_mask=gt_mask, objects=gts)
        out = scorer.score(dets)
        assert out["AP"] == 1.0 and out["AP50"] == 1.0 and out["AP75"] == 1.0 and out["AR"] == 1.0 and sorted(out["per_category"]) == [1]
        same_scores(out, ref.evaluate(cases.host_images({(1, 1): rows}, {(1, 1): [1] * 4}, dets, 0.1, iou_type, gt_mask, box), HW=H * W))
        # the ground truth below min_visib neither counts as missed (its detection left out: still 1.0) nor makes its detection false
        assert scorer.score({(1, 1): dets[(1, 1)][:3]})["AP"] == 1.0
        assert [r[2] for r in scorer.rows] == [False, False, False, True]
    strict = detections.DetectionScorer(table, iou_type=iou_type, gt_mask=gt_mask, objects=gts, min_visib=None)
    assert strict.score({(1, 1): dets[(1, 1)][:3]})["AR"] == 0.75                                  # without min_visib it is missed


@pytest.mark.parametrize("iou_type", ("segm", "bbox"))
def test_duplicates_wrong_categories_and_shifted_masks_score_what_the_restatement_scores(iou_type):
    gts, table = small_scene()
    H, W = gtinfo_cases.H, gtinfo_cases.W
    rows = table[(1, 1)]
    dets = {(1, 1): cases.perturbed_detections(rows, [1] * 4, H, W), (1, 7): [cases.detection(rows[0]["mask_visib"]["counts"], H, W, 1, 0.99)]}
    for max_dets in (100, 5):
        out = detections.DetectionScorer(table, iou_type=iou_type, objects=gts, max_dets=max_dets).score(dets)
        want = ref.evaluate(cases.host_images({(1, 1): rows}, {(1, 1): [1] * 4}, dets, 0.1, iou_type), max_dets=max_dets, HW=H * W)
        same_scores(out, want)
        assert 0.0 < out["AP"] < 1.0 and sorted(out["per_category"]) == [1]                       # category 8 has no ground truth: left out


@functools.lru_cache(maxsize=None)
def labelled_scene():
    """The two meshes of tests/golden/label_meshes.npz, two poses each, in ONE 240 x 320 frame: the ground truths of GroundTruthInfo
    (no depth: nothing occludes), the frame composed of MeshTemplates' renders, a bank of the same views.  The ViT is RANDOMLY
    INITIALISED: plumbing, not accuracy."""
    from gigapose_amd import render
    from gigapose_amd.vit import Dinov2ViT

    H, W = 240, 320
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_meshes.npz")
    with np.load(golden) as z:
        objs = [(z[f"{n}_vertices"], z[f"{n}_faces"], z[f"{n}_colours"]) for n in ("boxes", "ball")]
    rs = np.random.RandomState(77)
    spots = [[(-1.9, -1.1, 7.0), (1.9, 1.1, 7.2)], [(1.9, -1.1, 6.8), (-1.9, 1.1, 7.1)]]
    poses = [np.stack([pose(rotation(rs), t) for t in spots[o]]).astype(np.float32) for o in range(2)]
    templates = render.MeshTemplates(list(zip(objs, poses)), K=K_SMALL, device=DEV, H=H, W=W, znear=ZNEAR)
    vit = syn.fill_state_dict(Dinov2ViT(384, 12, 6), 31).eval().to(DEV)
    bank = proposals.DescriptorBank(vit)
    frame = np.zeros((3, H, W), np.uint8)
    gts = {(1, 1): []}
    for o in range(2):
        bank.add(o + 1, templates[o])
        rgba = templates.render(o)["rgba"].cpu().numpy()
        for t in range(2):
            drawn = rgba[t, ..., 3] > 0
            frame[:, drawn] = rgba[t, ..., :3][drawn].T
            gts[(1, 1)].append(dict(obj_id=o + 1, cam_R_m2c=poses[o][t, :3, :3].astype(np.float64).reshape(9).tolist(),
                                    cam_t_m2c=poses[o][t, :3, 3].astype(np.float64).tolist()))
    models = {o + 1: dict(vertices=objs[o][0], faces=objs[o][1]) for o in range(2)}
    table = gtinfo.GroundTruthInfo(models, {(1, 1): dict(cam_K=K_SMALL, size=(H, W))}, margin=0.0, znear=ZNEAR).compute(gts, masks=True)
    rows = table[(1, 1)]
    assert all(r["px_count_visib"] > 200 for r in rows)
    props = [dict(segmentation=r["mask_visib"]) for r in rows]
    props += [dict(segmentation=rows[0]["mask_visib"]), dict(segmentation=dict(size=[H, W], counts=cases.shifted(rows[1]["mask_visib"]["counts"], H, W, 4)))]
    return dict(H=H, W=W, vit=vit, bank=bank, frame=frame[None], gts=gts, table=table, props=props)


def test_labelled_proposals_go_straight_into_the_scorer():
    s = labelled_scene()
    H, W, rows = s["H"], s["W"], s["table"][(1, 1)]
    cats = [g["obj_id"] for g in s["gts"][(1, 1)]]
    for kw in (dict(), dict(nms_on="mask"), dict(nms_iou=(1, 1))):                                 # IoU > 1 never holds: nothing is suppressed
        dets = {(1, 1): proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=0.0, **kw).label(s["frame"], [s["props"]])[0]}
        assert len(dets[(1, 1)]) >= 4 and all(d["category_id"] in (1, 2) for d in dets[(1, 1)])
        for iou_type in ("segm", "bbox"):
            out = detections.DetectionScorer(s["table"], iou_type=iou_type, objects=s["gts"]).score(dets)
            same_scores(out, ref.evaluate(cases.host_images({(1, 1): rows}, {(1, 1): cats}, dets, 0.1, iou_type), HW=H * W))


def test_nms_on_mask_keeps_what_the_restatement_keeps_and_nms_on_box_is_the_labeller_as_it_was():
    s = labelled_scene()
    H, W = s["H"], s["W"]
    strip = lambda dets: [[(d["proposal"], d["category_id"], d["score"], d["bbox"], d["best_template"]) for d in im] for im in dets]      # noqa: E731
    plain = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=0.0)
    boxed = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=0.0, nms_on="box")
    assert strip(plain.label(s["frame"], [s["props"]])) == strip(boxed.label(s["frame"], [s["props"]])) and plain.report == boxed.report
    lists = [np.asarray(p["segmentation"]["counts"], np.int32) for p in s["props"]]
    cum, offsets = cases.pack_cum(lists)
    for kw in (dict(), dict(per_label=True), dict(nms_iou=(3, 4))):
        masked = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=0.0, nms_on="mask", **kw)
        dets = masked.label(s["frame"], [s["props"]])[0]
        d = masked.describe(s["frame"], [s["props"]])
        assert not d["mstatus"].any() and not d["dstatus"].any()
        order = np.argsort(-d["score"], kind="stable")
        num, den = masked.nms_iou
        fg, area, _ = ref.fg_scan(cum, offsets, H * W)
        a, b = ref.all_pairs(len(order))
        part, _ = ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), H * W, order[a], order[b])
        if masked.per_label:
            part = np.where(d["label"][order[a]] == d["label"][order[b]], part, 0)
        inter = np.zeros((len(order), len(order)), np.int64)
        inter[a, b] = part
        keep = label_ref.nms_keep(ref.sup_bits(inter, area[order], num, den), len(order))
        assert [x["proposal"] for x in dets] == order[keep.astype(bool)].tolist(), kw
        if not kw:
            assert ref.mask_nms(cum, offsets, H * W, order, num, den).tolist() == keep.tolist()
            assert len(dets) == 4 and masked.report["suppressed"] == 2                              # the duplicate and the shifted copy go
