"""GPU: hypothesis verification (libgigapose_verify.so, gigapose_amd/verify.py).

gpv_counts against the numpy restatement (gigapose_testing/verify_ref.py, written from the header and held to a set-based reading
and to what a verifier is for by tests/test_verify_host.py) bit for bit -- the rows of counts and the status words: on keys from
render.raster under every kind of box, on planted keys for every class and tolerance edge at the ends of waves and chunks, with
and without depth and masks, with shared, missing and bad masks, at the limits (65535 pairs in one call; a key buffer past 2^31
elements); the invariances an integer count must have; then HypothesisVerifier.score against the restatement over the numpy
rasteriser, and csv -> refine -> select -> csv -> PoseScorer on a scene whose coarse top-1 is wrong."""
import functools

import numpy as np
import pytest
import torch

from gigapose_testing import dist_ref, raster_ref, verify_ref
from gigapose_testing import refine_cases as rc
from gigapose_testing import verify_cases as cases

from gigapose_testing.gpu_cases import assert_bits, five_pairs
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = cases.H, cases.W


def packed(lists):
    """Run-length lists -> (run lengths, offsets, their prefix sums) on the host."""
    lists = [np.asarray(m, np.int32) for m in lists]
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int32)
    return np.concatenate(lists), offsets, np.concatenate([np.cumsum(m) for m in lists]).astype(np.int32)


def scanned(lists, h, w):
    """The lists as the ingest library leaves them on the device: (cum, offsets), cum checked against numpy's prefix sums."""
    from gigapose_amd import ingest

    runs, offsets, cum = packed(lists)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    offsets_d = _t(offsets)
    cum_d = ingest.RleDetectionPreprocessor().scan(_t(runs), offsets_d, h, w, err)
    assert err.item() == 0
    assert_bits(cum_d, cum, "gpi_rle_scan")
    return (cum_d, offsets_d), (cum, offsets)


def device_counts(vis, depth, frame, masks, det, box, tol):
    from gigapose_amd import verify

    rows, status = verify.counts(_t(np.asarray(vis)), None if depth is None else _t(np.asarray(depth, np.float32)),
                                 None if depth is None else _t(np.asarray(frame, np.int32)), masks, None if masks is None else _t(np.asarray(det, np.int32)),
                                 _t(np.asarray(box, np.int32)), _t(np.asarray(tol, np.float64)))
    return rows.cpu().numpy(), status.cpu().numpy()


def check_counts(what, vis, depth, frame, masks, det, box, tol):
    """masks: None or (device (cum, offsets), host (cum, offsets))."""
    got = device_counts(vis, depth, frame, None if masks is None else masks[0], det, box, tol)
    cum, offsets = (None, None) if masks is None else masks[1]
    want = verify_ref.counts(vis, depth, frame, cum, offsets, det, box, tol)
    assert_bits(got[0], want[0], f"{what}: counts")
    assert_bits(got[1], want[1], f"{what}: status")
    return want


# ---------------------------------------------------------------------------------------------- 1. keys from render.raster
@functools.lru_cache(maxsize=None)
def rendered():
    """Five pairs on two frames: the three starts about GT on frame 0, two about GT2 on frame 1; keys from render.raster; the
    masks of the two ground truths."""
    poses, vis = five_pairs()
    depth = np.stack([cases.truth(0)["depth"], cases.truth(1)["depth"]])
    n = len(poses)
    return dict(vis=vis, depth=depth, frame=np.asarray([0, 0, 0, 1, 1], np.int32), masks=scanned([cases.truth(0)["runs"], cases.truth(1)["runs"]], H, W),
                det=np.asarray([0, 0, 0, 1, 1], np.int32), tol=np.full(n, cases.COARSE_TOL * cases.SCALE))


def tight_boxes(vis):
    out = []
    for key in vis:
        ys, xs = np.nonzero(key != raster_ref.EMPTY_KEY)
        out.append((xs.min(), ys.min(), xs.max(), ys.max()))
    return np.asarray(out, np.int32)


def test_counts_on_rendered_keys_under_every_kind_of_box():
    r = rendered()
    n = len(r["vis"])
    whole = check_counts("whole frame", box=rc.whole_frame(n), **r)
    assert not whole[1].any() and (whole[0][:, 10:] == 0).all()
    for slot in (3, 4, 8, 9):                                     # agreeing pixels in the mask, the wall seen beside it, pixels of the mask that are missed
        assert whole[0][:, slot].all(), slot
    tight = tight_boxes(r["vis"])
    got = check_counts("tight", box=tight, **r)
    assert_bits(got[0][:, :8], whole[0][:, :8], "tight box = whole frame on the covered pixels")
    assert (got[0][:, 8] <= whole[0][:, 8]).all() and (got[0][:, 8] < whole[0][:, 8]).any()     # ... but not on the mask's pixels outside it
    cx, cy = (tight[:, 0] + tight[:, 2]) // 2, (tight[:, 1] + tight[:, 3]) // 2
    one = check_counts("1 x 1", box=np.stack([cx, cy, cx, cy], axis=1), **r)
    assert (one[0][:, :9].sum(axis=1) <= 1).all() and one[0][:, :9].any()
    for width in (63, 64, 65):
        check_counts(f"width {width}", box=np.stack([cx - 31, cy - 20, cx - 31 + width - 1, cy + 20], axis=1), **r)
    part = check_counts("partly outside", box=np.stack([cx, cy, cx + 500, cy + 500], axis=1), **r)
    assert part[0][:, :8].sum(axis=1).all()
    check_counts("negative corner", box=np.stack([cx - 500, cy - 500, cx, cy], axis=1), **r)
    for what, box in (("wholly outside, right", (W, 0, W + 50, H - 1)), ("wholly outside, above", (0, -40, W - 1, -1)), ("empty", (10, 10, 9, 20)),
                      ("inverted", (100, 80, 20, 10)), ("extreme", (-2 ** 31, -2 ** 31, -1, 2 ** 31 - 1))):
        got = check_counts(what, box=np.tile(np.asarray(box, np.int64).astype(np.int32), (n, 1)), **r)
        assert not got[0].any() and not got[1].any(), what
    mixed = tight.copy()
    mixed[1], mixed[3] = (5, 5, 4, 4), (0, 0, W - 1, H - 1)
    check_counts("a box of its own per pair", box=mixed, **r)


def random_frames(n, h, w, seed, fill=0.9):
    """Random keys (drawn depths 380 .. 420), one frame of measured depths within +-40 of the first pair's (some 0), and a random
    mask of short runs per pair."""
    rs = np.random.RandomState(seed)
    zr = rs.uniform(380, 420, (n, h, w)).astype(np.float32)
    vis = (zr.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 100, (n, h, w)).astype(np.uint64)
    vis[rs.uniform(size=vis.shape) > fill] = raster_ref.EMPTY_KEY
    depth = (zr[:1] + rs.uniform(-40, 40, (1, h, w))).astype(np.float32)
    depth[rs.uniform(size=depth.shape) > 0.95] = 0.0
    lists = [cases.mask_to_rle_counts(np.repeat(rs.uniform(size=(h, -(-w // 7))) > 0.5, 7, axis=1)[:, :w]) for _ in range(n)]
    return dict(vis=vis, depth=depth, frame=np.zeros(n, np.int32), masks=scanned(lists, h, w), det=np.arange(n, dtype=np.int32), tol=np.full(n, 12.5))


def test_counts_at_box_areas_around_the_workgroup_chunk():
    from gigapose_amd import verify

    C = verify.pixels_per_workgroup()
    w = 2 * C + 1                                                # a strip of one row: any area is a box (8193 pixels, fewer than 96 x 128)
    assert w <= H * W
    p = random_frames(4, 1, w, 11)
    boxes = np.asarray([(0, 0, C - 2, 0), (0, 0, C - 1, 0), (0, 0, C, 0), (0, 0, 2 * C, 0)], np.int32)
    want = check_counts("areas C-1, C, C+1, 2C+1", box=boxes, **p)
    assert (want[0][:, :8].sum(axis=1) > 0.8 * np.asarray([C - 1, C, C + 1, 2 * C + 1])).all() and want[0][:, :9].all()
    check_counts("boxes from x = C-1", box=boxes + np.asarray([C - 1, 0, 0, 0], np.int32), **p)
    p2 = random_frames(3, 3, C // 2 + 5, 12)                      # rows shorter than a chunk: a chunk spans rows, the mask's columns have 3 pixels
    check_counts("three rows", box=np.asarray([(0, 0, C // 2 + 4, 2), (1, 0, C // 2 + 3, 2), (7, 1, C // 2, 2)], np.int32), **p2)


# ---------------------------------------------------------------------------------------------- 2. planted keys
def test_counts_on_planted_keys_at_the_ends_of_waves_and_chunks():
    from gigapose_amd import verify

    C = verify.pixels_per_workgroup()
    h, w = 3, (2 * C + 1) // 3                                    # 3 x 2731 = 2C + 1 pixels: three chunks, the last of one pixel
    assert h * w == 2 * C + 1
    at = [0, 63, 64, C - 64, C - 1, C, 2 * C - 1, 2 * C]           # the first / last lane of a wave, the first / last pixel of a chunk
    kinds = cases.planted_pixels()
    vis, depth, lists, want_slot = [], [], [], []
    for i, (name, z, dm, cls) in enumerate(kinds):
        for bit in (0, 1):
            keys, d, mask, want = cases.planted_frame(h, w, [(idx % w, idx // w, i, bit) for idx in at])
            vis.append(keys), depth.append(d), lists.append(cases.mask_to_rle_counts(mask))
            want_slot.append(None if not want else next(iter(want)))
            assert all(v == {(idx % w, idx // w) for idx in at} for v in want.values()) and len(want) <= 1
    n = len(vis)
    assert n == 2 * len(kinds)
    masks = scanned(lists, h, w)
    got = check_counts("planted", np.stack(vis), np.stack(depth), np.arange(n, dtype=np.int32), masks, np.arange(n, dtype=np.int32),
                       rc.whole_frame(n, h, w), np.full(n, cases.PLANT_TOL))
    for row, slot in zip(got[0], want_slot):                     # ... and what the case says, not only what the restatement says
        want = np.zeros(9, np.int64)
        if slot is not None:
            want[slot] = len(at)
        assert row[:9].tolist() == want.tolist()
    assert {s for s in want_slot if s is not None} == set(range(9))
    special = dict(vis=np.stack(vis), depth=np.stack(depth), frame=np.arange(n, dtype=np.int32), masks=masks, det=np.arange(n, dtype=np.int32),
                   box=rc.whole_frame(n, h, w))
    zero = check_counts("tol = 0", tol=np.zeros(n), **special)
    assert zero[0][:, 2:4].sum() == 2 * len(at) and not zero[0][:, 9].any()               # r = 0 agrees at tol = 0 and adds no residual
    nan = check_counts("tol NaN", tol=np.full(n, np.nan), **special)
    assert not nan[0][:, 2:8].any() and nan[0][:, :2].sum() == 2 * len(at) * (len(kinds) - 1)
    check_counts("tol +inf", tol=np.full(n, np.inf), **special)


# ---------------------------------------------------------------------------------------------- 3. depth and mask combinations
def test_counts_with_and_without_depth_and_masks():
    r = rendered()
    n = len(r["vis"])
    box = rc.whole_frame(n)
    both = check_counts("both", box=box, **r)
    nodepth = check_counts("no depth", box=box, **dict(r, depth=None))
    assert not nodepth[0][:, 2:8].any() and not nodepth[0][:, 9].any()
    assert_bits(nodepth[0][:, 0] + nodepth[0][:, 1], both[0][:, :8].sum(axis=1), "covered")
    assert_bits(nodepth[0][:, 1], both[0][:, 1:8:2].sum(axis=1), "covered in the mask")
    nomask = check_counts("no masks", box=box, **dict(r, masks=None))
    assert not nomask[0][:, [1, 3, 5, 7, 8]].any()
    assert_bits(nomask[0][:, :8:2], both[0][:, :8:2] + both[0][:, 1:8:2], "the classes")
    assert_bits(nomask[0][:, 9], both[0][:, 9], "the residual does not depend on the mask")
    neither = check_counts("neither", box=box, **dict(r, depth=None, masks=None))
    assert_bits(neither[0][:, 0], both[0][:, :8].sum(axis=1), "covered")
    mixed = check_counts("det = -1 mixed with masked pairs", box=box, **dict(r, det=np.asarray([0, -1, 0, -7, 1], np.int32)))
    assert_bits(mixed[0][[1, 3]], nomask[0][[1, 3]], "a pair without a mask")
    assert_bits(mixed[0][[0, 2, 4]], both[0][[0, 2, 4]], "its neighbours")
    shared = dict(r, vis=r["vis"][[0, 1, 2, 0, 1]], frame=np.zeros(n, np.int32), det=np.zeros(n, np.int32))
    five = check_counts("five pairs sharing one det", box=box, **shared)
    assert_bits(five[0], both[0][[0, 1, 2, 0, 1]], "five pairs sharing one det")


def test_bad_masks_and_frames_set_their_bit_and_leave_the_neighbours_alone():
    r = rendered()
    n = len(r["vis"])
    box = rc.whole_frame(n)
    good = check_counts("good", box=box, **r)
    runs, offsets, cum = packed([cases.truth(0)["runs"], cases.truth(1)["runs"], cases.truth(0)["runs"]])
    cum[offsets[2] - 1] = -1                                     # detection 1: a list gpi_rle_scan marked bad
    masks = ((_t(cum), _t(offsets)), (cum, offsets))
    M, F = verify_ref.BAD_MASK, verify_ref.BAD_FRAME
    got = check_counts("a bad list, det >= D", box=box, **dict(r, masks=masks, det=np.asarray([0, 1, 3, 2, 2 ** 31 - 1], np.int32)))
    assert got[1].tolist() == [0, M, M, 0, M] and not got[0][[1, 2, 4]].any()
    assert_bits(got[0][0], good[0][0], "the neighbour of a bad mask")
    broken = offsets.copy()
    broken[1] = len(cum) + 5                                     # detection 0's slice leaves the array, detection 1's is inverted
    got = check_counts("slices outside the array", box=box, **dict(r, masks=((_t(cum), _t(broken)), (cum, broken)), det=np.asarray([0, 1, 2, 2, -1], np.int32)))
    assert got[1].tolist() == [M, M, 0, 0, 0]
    got = check_counts("a bad frame", box=box, **dict(r, frame=np.asarray([0, 2, 0, -1, 1], np.int32)))
    assert got[1].tolist() == [0, F, 0, F, 0] and not got[0][[1, 3]].any()
    assert_bits(got[0][[0, 2, 4]], good[0][[0, 2, 4]], "the neighbours of a bad frame")
    got = check_counts("both, and an empty box", box=np.tile(np.asarray([5, 5, 4, 4], np.int32), (n, 1)),
                       **dict(r, masks=masks, frame=np.asarray([0, 9, 0, 0, 0], np.int32), det=np.asarray([0, 1, 0, 0, 0], np.int32)))
    assert got[1].tolist() == [0, M | F, 0, 0, 0] and not got[0].any()          # the pair rules do not depend on the box


# ---------------------------------------------------------------------------------------------- 4. order and limits
def test_counts_invariances():
    r = rendered()
    n = len(r["vis"])
    box = tight_boxes(r["vis"])
    dm = r["masks"][0]
    whole = device_counts(r["vis"], r["depth"], r["frame"], dm, r["det"], box, r["tol"])
    order = np.asarray([3, 0, 4, 2, 1])
    got = device_counts(r["vis"][order], r["depth"], r["frame"][order], dm, r["det"][order], box[order], r["tol"][order])
    assert_bits(got[0], whole[0][order], "pairs permuted: counts")
    parts = [device_counts(r["vis"][a:b], r["depth"], r["frame"][a:b], dm, r["det"][a:b], box[a:b], r["tol"][a:b]) for a, b in ((0, 2), (2, 5))]
    assert_bits(np.concatenate([p[0] for p in parts]), whole[0], "pairs split over two calls")
    again = device_counts(r["vis"], r["depth"], r["frame"], dm, r["det"], box, r["tol"])
    assert_bits(again[0], whole[0], "a second run")


def test_counts_65535_pairs_in_one_call():
    n, reps = 5, 13107
    assert n * reps == 65535
    p = random_frames(n, 8, 16, 31, fill=0.8)
    box = np.asarray([(0, 0, 15, 7), (1, 1, 14, 6), (0, 0, 15, 3), (-3, 2, 40, 20), (4, 4, 4, 4)], np.int32)
    cum, offsets = p["masks"][1]
    want = verify_ref.counts(p["vis"], p["depth"], p["frame"], cum, offsets, p["det"], box, p["tol"])
    assert want[0][:4, :9].sum(axis=1).all()
    got = device_counts(np.tile(p["vis"], (reps, 1, 1)), p["depth"], np.tile(p["frame"], reps), p["masks"][0], np.tile(p["det"], reps), np.tile(box, (reps, 1)),
                        np.tile(p["tol"], reps))
    assert_bits(got[0], np.tile(want[0], (reps, 1)), "65535 pairs: counts")
    assert_bits(got[1], np.tile(want[1], reps), "65535 pairs: status")


def test_counts_addresses_a_key_buffer_past_2_to_the_31_elements():
    """513 pairs of 2048 x 2048: the LAST pair's keys begin 2^31 elements (16 GiB) into the buffer; only its box is non-empty, so
    only its plane is ever read and only its plane is initialised."""
    from gigapose_amd import verify

    n, side = 513, 2048
    assert (n - 1) * side * side >= 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    assert free > n * side * side * 8 + (1 << 30), "the device has too little free memory for this case"
    p = random_frames(1, 48, 48, 41)
    plane = np.full((side, side), raster_ref.EMPTY_KEY, np.uint64)
    plane[2000:2048, 2000:2048] = p["vis"][0]
    depth = np.zeros((1, side, side), np.float32)
    depth[0, 2000:2048, 2000:2048] = p["depth"][0]
    mask = np.zeros((side, side), bool)
    mask[1980:2030, 2010:2048] = True
    masks = scanned([cases.mask_to_rle_counts(mask)], side, side)
    box1 = np.asarray([[1990, 1995, 5000, 2047]], np.int32)
    want = verify_ref.counts(plane[None], depth, [0], *masks[1], [0], box1, [12.5])
    assert want[0][0, :9].all() and want[0][0, :8].sum() > 1000
    vis = torch.empty(n, side, side, dtype=torch.int64, device=DEV)
    vis[-1].copy_(_t(plane))
    box = np.tile(np.asarray([0, 0, -1, -1], np.int32), (n, 1))
    box[-1] = box1[0]
    rows, status = verify.counts(vis, _t(depth), _t(np.zeros(n, np.int32)), masks[0], _t(np.zeros(n, np.int32)), _t(box), _t(np.full(n, 12.5)))
    rows, status = rows.cpu().numpy(), status.cpu().numpy()
    del vis
    torch.cuda.empty_cache()
    assert not rows[:-1].any() and not status.any()
    assert_bits(rows[-1:], want[0], "the last pair: counts")


# ---------------------------------------------------------------------------------------------- 5. HypothesisVerifier
def estimates_of(poses, scene, im, obj, instance):
    return [dict(scene_id=scene, im_id=im, obj_id=obj, score=0.9 - 0.01 * i, R=p[:3, :3].copy(), t=p[:3, 3].copy(), instance_id=instance)
            for i, p in enumerate(poses)]


@functools.lru_cache(maxsize=None)
def scene():
    """The two instances on a frame each, six hypotheses per instance, the three WRONG ones first."""
    v, f = rc.mesh("boxes")
    models = {1: dict(vertices=v, faces=f, diameter=cases.SCALE)}
    cameras = {(1, i): dict(cam_K=cases.K, depth=cases.truth(i)["depth"]) for i in range(2)}
    est = estimates_of(cases.hypotheses(0), 1, 0, 1, 10) + estimates_of(cases.hypotheses(1), 1, 1, 1, 11)
    masks = {10 + i: cases.segmentation(cases.truth(i)["runs"]) for i in range(2)}
    return models, cameras, est, masks


def restated(est, tol, depth=True, masks=True, **kw):
    """The restatement's scores of the scene's estimates, in their order."""
    v, f = rc.mesh("boxes")
    poses = np.stack([rc.rigid(e["R"], e["t"]) for e in est])
    n = len(poses)
    frame = np.asarray([e["im_id"] for e in est], np.int32)
    sensor = np.stack([cases.truth(0)["depth"], cases.truth(1)["depth"]]) if depth else None
    lists = [cases.truth(0)["runs"], cases.truth(1)["runs"]] if masks else None
    return verify_ref.score_drawn(verify_ref.draw_poses(v, f, poses, cases.K, H, W), sensor, frame, lists, frame, rc.whole_frame(n), np.full(n, tol * cases.SCALE), **kw)


def check_scored(out, est, want, what):
    rows, status, s = want
    assert len(out) == len(est)
    for i, (o, e) in enumerate(zip(out, est)):
        assert_bits(o["counts"], rows[i], f"{what}: estimate {i}: counts")
        assert o["verify_status"] == int(status[i]) == 0
        for k in ("verify", "depth_fit", "iou", "residual"):
            assert np.float64(o[k]).tobytes() == np.float64(s[k][i]).tobytes(), (what, i, k, o[k], s[k][i])
        assert all(o[k] is e[k] or o[k] == e[k] for k in ("scene_id", "im_id", "obj_id", "score", "instance_id")) and o["R"] is e["R"]


def test_verifier_score_equals_the_restatement():
    from gigapose_amd import verify

    models, cameras, est, masks = scene()
    want = restated(est, cases.TOL)
    one = verify.HypothesisVerifier(models, cameras, box="frame").score(est, masks)
    check_scored(one, est, want, "one chunk")
    check_scored(verify.HypothesisVerifier(models, cameras, box="frame", pairs_per_call=2).score(est, masks), est, want, "chunks of 2")
    per_estimate = [masks[e["instance_id"]] for e in est]
    check_scored(verify.HypothesisVerifier(models, cameras, box="frame").score(est, per_estimate), est, want, "one mask per estimate")
    # the default box -- the projected model's, joined with the mask's -- holds every pixel that counts: the same rows
    check_scored(verify.HypothesisVerifier(models, cameras).score(est, masks), est, want, "the projected box")
    check_scored(verify.HypothesisVerifier(models, cameras, box="frame", occlusion_weight=1.0, min_points=400).score(est, masks), est,
                 restated(est, cases.TOL, occlusion_weight=1.0, min_points=400), "other parameters")
    check_scored(verify.HypothesisVerifier(models, cameras, tol=cases.COARSE_TOL).score(est), est, restated(est, cases.COARSE_TOL, masks=False), "depth only")
    rgb = {k: dict(cam_K=c["cam_K"]) for k, c in cameras.items()}
    check_scored(verify.HypothesisVerifier(models, rgb).score(est, masks), est, restated(est, cases.TOL, depth=False), "masks only")
    from gigapose_amd import rle_strings

    strings = {k: dict(size=m["size"], counts=rle_strings.rle_string_from_counts(m["counts"])) for k, m in masks.items()}
    check_scored(verify.HypothesisVerifier(models, cameras, box="frame").score(est, strings), est, want, "compressed strings")


def test_right_hypotheses_rank_first_through_the_kernels_before_and_after_refinement():
    from gigapose_amd import refine, verify

    models, cameras, est, masks = scene()
    v = models[1]["vertices"]
    refined = refine.DepthRefiner(models, cameras, iters=rc.ITERS, box="frame").refine(est)
    rgb = {k: dict(cam_K=c["cam_K"]) for k, c in cameras.items()}
    for what, hyps, tol in (("before", est, cases.COARSE_TOL), ("after", refined, cases.TOL)):
        for mode, verifier, m in (("depth", verify.HypothesisVerifier(models, cameras, tol=tol), None), ("mask", verify.HypothesisVerifier(models, rgb, tol=tol), masks),
                                  ("both", verify.HypothesisVerifier(models, cameras, tol=tol), masks)):
            s = np.asarray([o["verify"] for o in verifier.score(hyps, m)]).reshape(2, 6)
            print(what, mode, np.round(s, 3))
            assert (s[:, 3:].min(axis=1) > s[:, :3].max(axis=1)).all(), (what, mode)          # (a)
    verifier = verify.HypothesisVerifier(models, cameras)
    chosen = verify.refine_and_select(refine.DepthRefiner(models, cameras, iters=rc.ITERS, box="frame"), verifier, est, masks)
    assert [e["instance_id"] for e in chosen] == [10, 11]
    for which, e in enumerate(chosen):                           # (e), (f): a right one, below 1 % of its start; the coarse top-1 is not
        k = round((0.9 - e["score"]) / 0.01)
        assert k >= 3 and e["score"] == est[6 * which + k]["score"]
        assert rc.deviation(v, rc.rigid(e["R"], e["t"]), cases.GTS[which]) < 0.01 * rc.deviation(v, cases.hypotheses(which)[k], cases.GTS[which])
        top1 = refined[6 * which]
        assert not rc.deviation(v, rc.rigid(top1["R"], top1["t"]), cases.GTS[which]) < 0.01 * rc.deviation(v, cases.hypotheses(which)[0], cases.GTS[which])
    ranked = verifier.rank(refined, masks, score="verify")
    assert [e["instance_id"] for e in ranked] == [10] * 6 + [11] * 6
    assert all(a["score"] >= b["score"] for a, b in zip(ranked[:5], ranked[1:6])) and all(a["score"] >= b["score"] for a, b in zip(ranked[6:11], ranked[7:]))
    tied = [dict(est[3], score=0.2), dict(est[3], score=0.7), dict(est[3], score=0.7), dict(est[0], score=0.9)]       # an exact tie of the verification score
    assert verifier.select(tied, masks)[0]["score"] == 0.7 and [e["score"] for e in verifier.rank(tied, masks)] == [0.7, 0.7, 0.2, 0.9]


def test_selected_hypotheses_score_above_the_refined_top_1(tmp_path):
    """A MultiHypothesis.csv written by inout.py whose hypothesis 0 is wrong for both detections: csv -> refine all -> select ->
    csv -> PoseScorer.score_csv, against refining the top-1 file alone; and the same with hypothesis 0 right."""
    from gigapose_amd import evaluate, inout, refine, verify

    v, f = rc.mesh("boxes")
    diameter = dist_ref.diameter(v)
    models = {1: dict(vertices=v, faces=f, diameter=diameter)}
    cameras = {(1, i): dict(cam_K=cases.K, depth=cases.truth(i)["depth"]) for i in range(2)}
    targets = [dict(scene_id=1, im_id=i, obj_id=1, inst_count=1) for i in range(2)]
    gts = {(1, i): [dict(obj_id=1, cam_R_m2c=g[:3, :3].reshape(-1), cam_t_m2c=g[:3, 3])] for i, g in enumerate(cases.GTS)}
    scorer = evaluate.PoseScorer(models, targets, gts, cameras)
    refiner = refine.DepthRefiner(models, cameras, iters=rc.ITERS)
    verifier = verify.HypothesisVerifier(models, cameras)
    masks = {i: cases.segmentation(cases.truth(i)["runs"]) for i in range(2)}
    results = {}
    for what, order in (("wrong first", [0, 1, 2, 3, 4, 5]), ("right first", [4, 0, 1, 2, 3, 5])):
        d = tmp_path / what.replace(" ", "_")
        d.mkdir()
        poses = np.stack([cases.hypotheses(i)[order] for i in range(2)]).astype(np.float32)
        np.savez(d / "0.npz", poses=poses, scores=np.tile(0.9 - 0.1 * np.arange(6, dtype=np.float32), (2, 1)), object_id=np.asarray([1, 1]),
                 scene_id=np.asarray([1, 1]), im_id=np.asarray([0, 1]), time=np.asarray([0.1, 0.1]), detection_time=np.asarray([0.2, 0.2]))
        top1, multi = inout.save_predictions_from_batched_predictions(str(d), "ycbv", "gigapose", "run", False)
        hyps = verify.read_hypotheses(multi)
        assert [e["instance_id"] for e in hyps] == [0] * 6 + [1] * 6
        chosen = verify.refine_and_select(refiner, verifier, hyps, masks)
        assert len(chosen) == 2
        selected = scorer.score_csv(refine.write_estimates(d / "selected.csv", chosen))
        single = scorer.score_csv(refine.write_estimates(d / "top1_refined.csv", refiner.refine(verify.read_hypotheses(top1))))
        results[what] = (selected, single)
        print(what, "selected", {k: selected[k] for k in ("ar_mssd", "ar_mspd")}, "refined top-1", {k: single[k] for k in ("ar_mssd", "ar_mspd")})
        assert selected["ar_mssd"] >= single["ar_mssd"] and selected["ar_mspd"] >= single["ar_mspd"]
    selected, single = results["wrong first"]
    assert selected["ar_mssd"] > single["ar_mssd"] and selected["ar_mspd"] > single["ar_mspd"]
    assert selected["ar_mssd"] == 1.0 and selected["ar_mspd"] == 1.0
