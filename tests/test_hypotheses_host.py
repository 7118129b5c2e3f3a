"""gigapose_amd/hypotheses.py on the host (no GPU): the functions DepthRefiner, HypothesisVerifier and MaskRefiner share, held to
things that cannot share their mistakes -- a dense decode by a plain loop, the two mask forms against each other, the order of
first appearance written out, and the errors the three classes (and PoseScorer) raise through the camera table."""
import numpy as np
import pytest

from gigapose_amd import hypotheses, maskfit, refine, verify
from gigapose_amd.ingest import mask_to_rle_counts
from gigapose_testing import maskfit_cases as mc
from gigapose_testing import refine_cases as rc

EST = dict(scene_id=1, im_id=1, obj_id=1, score=0.5, R=np.eye(3), t=np.asarray([0.0, 0.0, 100.0]))
MODELS = {1: dict(vertices=np.zeros((5, 3), np.float32), faces=np.zeros((4, 3), np.int32), diameter=10.0),
          2: dict(vertices=np.zeros((5, 3), np.float32), faces=np.zeros((4, 3), np.int32), diameter=20.0)}


def rgb_table(**camera):
    return hypotheses.CameraTable("test", {(1, 1): dict(cam_K=rc.K, **camera)}, "ignored")


def dense_reading(runs, h, w):
    """Pixel by pixel: the runs alternate zeros and ones over the column-major pixels -> (dense mask, area, box x0 y0 x1 y1)."""
    dense, p, value = np.zeros((h, w), bool), 0, False
    for r in runs:
        for _ in range(int(r)):
            dense[p % h, p // h] = value
            p += 1
        value = not value
    assert p == h * w
    area, box = 0, [w, h, -1, -1]
    for y in range(h):
        for x in range(w):
            if dense[y, x]:
                area += 1
                box = [min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)]
    return dense, area, box


def test_mask_areas_and_boxes_equal_a_dense_decode_by_a_plain_loop():
    cases = [(name, mask_to_rle_counts(m), m) for name, m in mc.host_masks()]
    cases.append(("zero-length runs",) + mc.zero_length_runs())
    cases.append(("all zero", np.asarray([6 * 4], np.int32), np.zeros((6, 4), bool)))
    names = [c[0] for c in cases]
    assert "wraps three columns" in names and "ends at a column's end" in names and "empty" in names
    for name, runs, mask in cases:
        h, w = mask.shape
        seg = dict(size=[h, w], counts=[int(c) for c in runs])
        table = rgb_table()
        packed, offsets, det, area, boxes = hypotheses.pack_masks("test", [EST, EST], [seg, None], table)
        dense, want_area, want_box = dense_reading(packed[offsets[0]:offsets[1]], h, w)
        assert (dense == mask).all(), name
        assert (table.H, table.W) == (h, w) and det.tolist() == [0, -1], name                 # the size arrives with the first mask
        assert area[0] == want_area and np.isnan(area[1]), name
        assert boxes.tolist() == [want_box], name
        if not want_area:
            assert boxes.tolist() == [[w, h, -1, -1]], name


def test_both_mask_forms_and_a_shared_dictionary_give_the_same_detections():
    a, b = (dict(size=[5, 7], counts=[int(c) for c in mask_to_rle_counts(m)]) for m in (dict(mc.host_masks())["wraps three columns"], dict(mc.host_masks())["full"]))
    est = [dict(EST, instance_id=i) for i in (0, 0, 1, 2, 1)]
    by_id = hypotheses.pack_masks("test", est, {0: a, 1: b}, rgb_table())
    per_estimate = hypotheses.pack_masks("test", est, [a, a, b, None, b], rgb_table())
    assert by_id[2].tolist() == per_estimate[2].tolist() == [0, 0, 1, -1, 1]                 # None, or an instance without a mask: -1
    for x, y in zip(by_id, per_estimate):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    copies = hypotheses.pack_masks("test", est[:2], [a, dict(a)], rgb_table())               # equal, but not the same dictionary
    assert copies[2].tolist() == [0, 1] and len(copies[1]) == 3
    none = hypotheses.pack_masks("test", est[:2], [None, None], rgb_table(size=(5, 7)))
    assert none[2].tolist() == [-1, -1] and len(none[0]) == 0 and np.isnan(none[3]).all()
    with pytest.raises(ValueError, match="frame size is unknown"):
        hypotheses.pack_masks("test", est[:2], [None, None], rgb_table())


def test_groups_come_in_order_of_first_appearance():
    K2 = rc.K * np.asarray([1.5, 1, 1, 1, 1.5, 1, 1, 1, 1])
    table = hypotheses.CameraTable("test", {(1, 1): dict(cam_K=rc.K), (1, 2): dict(cam_K=K2), (2, 7): dict(cam_K=rc.K)}, "ignored")
    order = [(2, (1, 2)), (1, (1, 1)), (2, (1, 1)), (1, (2, 7)), (2, (1, 2)), (1, (1, 2)), (2, (2, 7)), (1, (1, 1))]
    est = [dict(EST, obj_id=o, scene_id=s, im_id=i) for o, (s, i) in order]
    groups = hypotheses.grouped("test", est, table, MODELS)
    assert [(k[0], k[1] == K2.tobytes(), idx) for k, idx in groups] == [(2, True, [0, 4]), (1, False, [1, 3, 7]), (2, False, [2, 6]), (1, True, [5])]
    with pytest.raises(ValueError, match=r"estimate 1: image \(1, 3\) has no camera"):
        hypotheses.grouped("test", est[:1] + [dict(EST, im_id=3, obj_id=3)], table, MODELS)    # the camera is judged before the model
    with pytest.raises(ValueError, match="estimate 0: object 3 has no model"):
        hypotheses.grouped("test", [dict(EST, obj_id=3)], table, MODELS)


def test_each_depth_policy_raises_what_its_classes_raise():
    d = np.zeros((8, 8), np.float32)
    both, mixed = {(1, 1): dict(cam_K=rc.K, depth=d), (1, 2): dict(cam_K=rc.K, depth=d)}, {(1, 1): dict(cam_K=rc.K, depth=d), (1, 2): dict(cam_K=rc.K)}
    differ = {(1, 1): dict(cam_K=rc.K, depth=d), (1, 2): dict(cam_K=rc.K, depth=np.zeros((8, 9), np.float32))}
    # required: DepthRefiner, PoseScorer
    t = hypotheses.CameraTable("test", both)
    assert (t.H, t.W, t.frames, t.index, t.depth_host.shape) == (8, 8, [(1, 1), (1, 2)], {(1, 1): 0, (1, 2): 1}, (2, 8, 8))
    for make in (lambda c: hypotheses.CameraTable("test", c), lambda c: refine.DepthRefiner(MODELS, c)):
        with pytest.raises(KeyError, match="depth"):
            make(mixed)
        with pytest.raises(ValueError, match="differ in size"):
            make(differ)
        with pytest.raises(ValueError, match="no cameras"):
            make({})
    # all or none: HypothesisVerifier
    for make in (lambda c: hypotheses.CameraTable("test", c, "all_or_none"), lambda c: verify.HypothesisVerifier(MODELS, c)):
        with pytest.raises(ValueError, match="for every frame or for none"):
            make(mixed)
        with pytest.raises(ValueError, match="differ in size"):
            make(differ)
        assert (make(both).H, make(both).W) == (8, 8)
        rgb = make({(1, 1): dict(cam_K=rc.K), (1, 2): dict(cam_K=rc.K, size=(6, 9))})
        assert (rgb.H, rgb.W) == (6, 9)
        with pytest.raises(ValueError, match="frame sizes differ: 6 x 9 and 8 x 8"):
            make({(1, 1): dict(cam_K=rc.K, depth=d, size=(6, 9))})
    assert hypotheses.CameraTable("test", {(1, 1): dict(cam_K=rc.K)}, "all_or_none").depth_host is None
    # ignored: MaskRefiner
    for make in (lambda c: hypotheses.CameraTable("test", c, "ignored"), lambda c: maskfit.MaskRefiner(MODELS, c)):
        for cameras in (mixed, differ):
            assert make(cameras).H is None
        assert (make({(1, 1): dict(cam_K=rc.K, depth=d, size=(6, 9))}).H, make({(1, 1): dict(cam_K=rc.K, depth=d, size=(6, 9))}).W) == (6, 9)
    assert hypotheses.CameraTable("test", both, "ignored").depth_host is None
    # the pixel limit
    with pytest.raises(ValueError, match="2\\^22"):
        hypotheses.CameraTable("test", {(1, 1): dict(cam_K=rc.K, size=(2048, 2049))}, "ignored")
    assert hypotheses.CameraTable("test", {(1, 1): dict(cam_K=rc.K, size=(2048, 2049))}, "ignored", max_pixels=None).W == 2049
    with pytest.raises(ValueError, match="diameter"):
        hypotheses.check_models("test", {1: dict(MODELS[1], diameter=0.0)})
