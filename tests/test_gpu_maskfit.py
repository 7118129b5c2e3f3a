"""GPU: the silhouette fit (libgigapose_maskfit.so, gigapose_amd/maskfit.py).

gpm_moments, gpm_mask_moments and gpm_update against the restatement (gigapose_testing/maskfit_ref.py, written from the header
and held to independent readings and to what a fit is for by tests/test_maskfit_host.py) bit for bit: on keys from render.raster
under every kind of box, at box areas around the workgroup's chunk, on pixels planted at the ends of waves and chunks and on each
edge of the box, with shared, missing and bad masks, at the limits (65535 pairs in one call; a key buffer past 2^31 elements);
the mask's moments on the host cases and on lists that came through gpi_rle_scan; the step on the planted rows; then
MaskRefiner.refine against the restatement's loop over the numpy rasteriser, and fit -> refine -> select."""
import functools

import numpy as np
import pytest
import torch

from gigapose_amd import maskfit
from gigapose_testing import maskfit_cases as mc
from gigapose_testing import maskfit_ref as ref
from gigapose_testing import raster_ref
from gigapose_testing import refine_cases as rc
from gigapose_testing import verify_cases as vc

from gigapose_testing.gpu_cases import assert_bits, five_pairs
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = mc.H, mc.W


def scanned(lists, h, w):
    """The lists as the ingest library leaves them on the device: (cum, offsets), cum checked against numpy's prefix sums."""
    from gigapose_amd import ingest

    cum, offsets = ref.cum_of(lists)
    runs = np.concatenate([np.asarray(m, np.int32) for m in lists])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    offsets_d = _t(offsets)
    cum_d = ingest.RleDetectionPreprocessor().scan(_t(runs), offsets_d, h, w, err)
    assert err.item() == 0
    assert_bits(cum_d, cum, "gpi_rle_scan")
    return (cum_d, offsets_d), (cum, offsets)


def device_moments(vis, masks, det, box):
    rows, status = maskfit.moments(_t(np.asarray(vis)), masks, _t(np.asarray(det, np.int32)), _t(np.asarray(box, np.int32)))
    return rows.cpu().numpy(), status.cpu().numpy()


def check_moments(what, vis, masks, det, box):
    """masks: (device (cum, offsets), host (cum, offsets))."""
    got = device_moments(vis, masks[0], det, box)
    want = ref.moments(vis, *masks[1], det, box)
    assert_bits(got[0], want[0], f"{what}: rows")
    assert_bits(got[1], want[1], f"{what}: status")
    return want


# ---------------------------------------------------------------------------------------------- 1. keys from render.raster
@functools.lru_cache(maxsize=None)
def rendered():
    """Five pairs: the three starts about GT, two about GT2; keys from render.raster; the masks of the two ground truths."""
    _, vis = five_pairs()
    return dict(vis=vis, masks=scanned([vc.truth(0)["runs"], vc.truth(1)["runs"]], H, W), det=np.asarray([0, 0, 0, 1, 1], np.int32))


def tight_boxes(vis):
    out = []
    for key in vis:
        ys, xs = np.nonzero(key != raster_ref.EMPTY_KEY)
        out.append((xs.min(), ys.min(), xs.max(), ys.max()))
    return np.asarray(out, np.int32)


def test_moments_on_rendered_keys_under_every_kind_of_box():
    r = rendered()
    n = len(r["vis"])
    whole = check_moments("whole frame", box=rc.whole_frame(n), **r)
    assert not whole[1].any() and (whole[0][:, 8:] == 0).all() and whole[0][:, :7].all() and not whole[0][:, 7].any()
    tight = tight_boxes(r["vis"])
    got = check_moments("tight", box=tight, **r)
    assert_bits(got[0][:, :7], whole[0][:, :7], "tight box = whole frame on the covered pixels")
    assert (got[0][:, 7] >= 4).all()
    cx, cy = (tight[:, 0] + tight[:, 2]) // 2, (tight[:, 1] + tight[:, 3]) // 2
    one = check_moments("1 x 1", box=np.stack([cx, cy, cx, cy], axis=1), **r)
    assert (one[0][:, 0] <= 1).all() and one[0][:, 0].any()
    for width in (63, 64, 65):
        check_moments(f"width {width}", box=np.stack([cx - 31, cy - 20, cx - 31 + width - 1, cy + 20], axis=1), **r)
    part = check_moments("partly outside", box=np.stack([cx, cy, cx + 500, cy + 500], axis=1), **r)
    assert part[0][:, 0].all()
    check_moments("negative corner", box=np.stack([cx - 500, cy - 500, cx, cy], axis=1), **r)
    for what, box in (("wholly outside, right", (W, 0, W + 50, H - 1)), ("wholly outside, above", (0, -40, W - 1, -1)), ("empty", (10, 10, 9, 20)),
                      ("inverted", (100, 80, 20, 10)), ("extreme", (-2 ** 31, -2 ** 31, -1, 2 ** 31 - 1))):
        got = check_moments(what, box=np.tile(np.asarray(box, np.int64).astype(np.int32), (n, 1)), **r)
        assert not got[0].any() and not got[1].any(), what
    mixed = tight.copy()
    mixed[1], mixed[3] = (5, 5, 4, 4), (0, 0, W - 1, H - 1)
    check_moments("a box of its own per pair", box=mixed, **r)


def random_frames(n, h, w, seed, fill=0.9):
    """Random keys and a random mask of short runs per pair."""
    rs = np.random.RandomState(seed)
    zr = rs.uniform(380, 420, (n, h, w)).astype(np.float32)
    vis = (zr.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 100, (n, h, w)).astype(np.uint64)
    vis[rs.uniform(size=vis.shape) > fill] = raster_ref.EMPTY_KEY
    lists = [vc.mask_to_rle_counts(np.repeat(rs.uniform(size=(h, -(-w // 7))) > 0.5, 7, axis=1)[:, :w]) for _ in range(n)]
    return dict(vis=vis, masks=scanned(lists, h, w), det=np.arange(n, dtype=np.int32))


def test_moments_at_box_areas_around_the_workgroup_chunk():
    C = maskfit.pixels_per_workgroup()
    w = 2 * C + 1                                                # a strip of one row: any area is a box
    p = random_frames(4, 1, w, 11)
    boxes = np.asarray([(0, 0, C - 2, 0), (0, 0, C - 1, 0), (0, 0, C, 0), (0, 0, 2 * C, 0)], np.int32)
    want = check_moments("areas C-1, C, C+1, 2C+1", box=boxes, **p)
    assert (want[0][:, 0] > 0.8 * np.asarray([C - 1, C, C + 1, 2 * C + 1])).all() and want[0][:, [0, 1, 3, 6]].all()
    check_moments("boxes from x = C-1", box=boxes + np.asarray([C - 1, 0, 0, 0], np.int32), **p)
    p2 = random_frames(3, 3, C // 2 + 5, 12)                      # rows shorter than a chunk: a chunk spans rows, the mask's columns have 3 pixels
    check_moments("three rows", box=np.asarray([(0, 0, C // 2 + 4, 2), (1, 0, C // 2 + 3, 2), (7, 1, C // 2, 2)], np.int32), **p2)


# ---------------------------------------------------------------------------------------------- 2. planted pixels
def test_moments_on_pixels_planted_at_the_ends_of_waves_and_chunks():
    C = maskfit.pixels_per_workgroup()
    h, w = 3, (2 * C + 1) // 3                                    # 3 x 2731 = 2C + 1 pixels: three chunks, the last of one pixel
    assert h * w == 2 * C + 1
    at = [0, 63, 64, C - 64, C - 1, C, 2 * C - 1, 2 * C]           # the first / last lane of a wave, the first / last pixel of a chunk
    vis, lists, want = [], [], []
    for covered in (0, 1):
        for bit in (0, 1):
            for only in [None] + at:
                keys, mask = np.full((h, w), raster_ref.EMPTY_KEY, np.uint64), np.zeros((h, w), bool)
                xs, ys = [i % w for i in at if only in (None, i)], [i // w for i in at if only in (None, i)]
                if covered:
                    keys[ys, xs] = vc.key_of(300.0, 7)
                mask[ys, xs] = bool(bit)
                vis.append(keys), lists.append(vc.mask_to_rle_counts(mask))
                x, y = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
                want.append([0] * 8 if not covered else [len(x), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), bit * len(x), 0])
    n = len(vis)
    got = check_moments("planted", np.stack(vis), scanned(lists, h, w), np.arange(n, dtype=np.int32), rc.whole_frame(n, h, w))
    assert got[0][:, :8].tolist() == want                         # ... and what the case says, not only what the restatement says


def test_the_box_edge_counter_on_each_edge_and_on_frame_edges():
    h, w = 12, 16
    full = np.full((h, w), vc.key_of(300.0, 1), np.uint64)
    mask = np.zeros((h, w), bool)
    mask[4:9, 5:12] = True
    masks = scanned([vc.mask_to_rle_counts(mask)], h, w)
    boxes = [(3, 2, 10, 8), (0, 0, w - 1, h - 1), (0, 2, 10, 8), (3, 0, 10, 8), (3, 2, w - 1, 8), (3, 2, 10, h - 1), (0, 0, 10, 8), (3, 2, 40, 40), (5, 5, 5, 5), (0, 3, 0, 3)]
    want = [2 * 8 + 2 * 7 - 4, 0, 7 + 11 + 11 - 2, 9 + 9 + 8 - 2, 7 + 13 + 13 - 2, 10 + 10 + 8 - 2, 9 + 11 - 1, 10 + 13 - 1, 1, 1]      # the sides that count, less shared corners
    n = len(boxes)
    got = check_moments("a full frame", np.tile(full, (n, 1, 1)), masks, np.zeros(n, np.int32), np.asarray(boxes, np.int32))
    assert got[0][:, ref.EDGE].tolist() == want
    single = []                                                   # one covered pixel in the middle of each edge of the box (3, 2, 10, 8), at a corner, inside
    for x, y in ((3, 5), (10, 5), (6, 2), (6, 8), (3, 2), (10, 8), (6, 5)):
        keys = np.full((h, w), raster_ref.EMPTY_KEY, np.uint64)
        keys[y, x] = vc.key_of(300.0, 2)
        single.append(keys)
    got = check_moments("single pixels", np.stack(single), masks, np.zeros(7, np.int32), np.tile(np.asarray(boxes[0], np.int32), (7, 1)))
    assert got[0][:, ref.EDGE].tolist() == [1, 1, 1, 1, 1, 1, 0] and got[0][:, 0].tolist() == [1] * 7


# ---------------------------------------------------------------------------------------------- 3. masks: shared, missing, bad
def test_shared_missing_and_bad_masks():
    r = rendered()
    n = len(r["vis"])
    box = rc.whole_frame(n)
    good = check_moments("good", box=box, **r)
    shared = check_moments("five pairs sharing one det", box=box, **dict(r, vis=r["vis"][[0, 1, 2, 0, 1]], det=np.zeros(n, np.int32)))
    assert_bits(shared[0], good[0][[0, 1, 2, 0, 1]], "five pairs sharing one det")
    other = check_moments("the other mask", box=box, **dict(r, det=np.asarray([1, 1, 1, 0, 0], np.int32)))
    assert_bits(other[0][:, :6], good[0][:, :6], "the covered pixels do not depend on the mask")
    assert (other[0][:, 6] != good[0][:, 6]).any()
    missing = check_moments("det = -1 mixed with masked pairs", box=box, **dict(r, det=np.asarray([0, -1, 0, -7, 1], np.int32)))
    assert missing[1].tolist() == [0, ref.NO_MASK, 0, ref.NO_MASK, 0] and not missing[0][[1, 3]].any()
    assert_bits(missing[0][[0, 2, 4]], good[0][[0, 2, 4]], "its neighbours")
    cum, offsets = ref.cum_of([vc.truth(0)["runs"], vc.truth(1)["runs"], vc.truth(0)["runs"]])
    cum[offsets[2] - 1] = -1                                     # detection 1: a list gpi_rle_scan marked bad
    masks = ((_t(cum), _t(offsets)), (cum, offsets))
    B = ref.BAD_MASK
    got = check_moments("a bad list, det >= D", box=box, **dict(r, masks=masks, det=np.asarray([0, 1, 3, 2, 2 ** 31 - 1], np.int32)))
    assert got[1].tolist() == [0, B, B, 0, B] and not got[0][[1, 2, 4]].any()
    assert_bits(got[0][0], good[0][0], "the neighbour of a bad mask")
    broken = offsets.copy()
    broken[1] = len(cum) + 5                                     # detection 0's slice leaves the array, detection 1's is inverted
    got = check_moments("slices outside the array", box=box, **dict(r, masks=((_t(cum), _t(broken)), (cum, broken)), det=np.asarray([0, 1, 2, 2, -1], np.int32)))
    assert got[1].tolist() == [B, B, 0, 0, ref.NO_MASK]
    got = check_moments("bad, and an empty box", box=np.tile(np.asarray([5, 5, 4, 4], np.int32), (n, 1)), **dict(r, masks=masks, det=np.asarray([0, 1, -1, 0, 0], np.int32)))
    assert got[1].tolist() == [0, B, ref.NO_MASK, 0, 0] and not got[0].any()       # the pair rules do not depend on the box
    mm, mstatus = maskfit.mask_moments(masks[0], H, W)
    want = ref.mask_moments(cum, offsets, H, W)
    assert_bits(mm, want[0], "mask_moments with a bad list")
    assert_bits(mstatus, want[1], "mstatus")
    assert want[1].tolist() == [0, B, 0] and not want[0][1].any()


# ---------------------------------------------------------------------------------------------- 4. order and limits
def test_moments_invariances():
    r = rendered()
    box = tight_boxes(r["vis"])
    dm = r["masks"][0]
    whole = device_moments(r["vis"], dm, r["det"], box)
    order = np.asarray([3, 0, 4, 2, 1])
    got = device_moments(r["vis"][order], dm, r["det"][order], box[order])
    assert_bits(got[0], whole[0][order], "pairs permuted")
    parts = [device_moments(r["vis"][a:b], dm, r["det"][a:b], box[a:b]) for a, b in ((0, 2), (2, 5))]
    assert_bits(np.concatenate([p[0] for p in parts]), whole[0], "pairs split over two calls")
    assert_bits(device_moments(r["vis"], dm, r["det"], box)[0], whole[0], "a second run")


def test_moments_65535_pairs_in_one_call():
    n, reps = 5, 13107
    assert n * reps == 65535
    p = random_frames(n, 8, 16, 31, fill=0.8)
    box = np.asarray([(0, 0, 15, 7), (1, 1, 14, 6), (0, 0, 15, 3), (-3, 2, 40, 20), (4, 4, 4, 4)], np.int32)
    want = ref.moments(p["vis"], *p["masks"][1], p["det"], box)
    assert want[0][:4, :7].all()
    got = device_moments(np.tile(p["vis"], (reps, 1, 1)), p["masks"][0], np.tile(p["det"], reps), np.tile(box, (reps, 1)))
    assert_bits(got[0], np.tile(want[0], (reps, 1)), "65535 pairs: rows")
    assert_bits(got[1], np.tile(want[1], reps), "65535 pairs: status")


def test_moments_addresses_a_key_buffer_past_2_to_the_31_elements():
    """513 pairs of 2048 x 2048: the LAST pair's keys begin 2^31 elements (16 GiB) into the buffer; only its box is non-empty, so
    only its plane is ever read and only its plane is initialised."""
    n, side = 513, 2048
    assert (n - 1) * side * side >= 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    assert free > n * side * side * 8 + (1 << 30), "the device has too little free memory for this case"
    p = random_frames(1, 48, 48, 41)
    plane = np.full((side, side), raster_ref.EMPTY_KEY, np.uint64)
    plane[2000:2048, 2000:2048] = p["vis"][0]
    mask = np.zeros((side, side), bool)
    mask[1980:2030, 2010:2048] = True
    masks = scanned([vc.mask_to_rle_counts(mask)], side, side)
    box1 = np.asarray([[2005, 2003, 5000, 2047]], np.int32)            # its left and upper edge cut through the drawing
    want = ref.moments(plane[None], *masks[1], [0], box1)
    assert want[0][0, :8].all() and want[0][0, 0] > 1000
    vis = torch.empty(n, side, side, dtype=torch.int64, device=DEV)
    vis[-1].copy_(_t(plane))
    box = np.tile(np.asarray([0, 0, -1, -1], np.int32), (n, 1))
    box[-1] = box1[0]
    rows, status = maskfit.moments(vis, masks[0], _t(np.zeros(n, np.int32)), _t(box))
    rows, status = rows.cpu().numpy(), status.cpu().numpy()
    del vis
    torch.cuda.empty_cache()
    assert not rows[:-1].any() and not status.any()
    assert_bits(rows[-1:], want[0], "the last pair: rows")


# ---------------------------------------------------------------------------------------------- 5. the mask's moments
def check_mask_moments(what, lists, dense, h, w):
    masks = scanned(lists, h, w)
    mm, mstatus = maskfit.mask_moments(masks[0], h, w)
    want = ref.mask_moments(*masks[1], h, w)
    assert_bits(mm, want[0], f"{what}: mm")
    assert_bits(mstatus, want[1], f"{what}: mstatus")
    assert not want[1].any()
    for d, m in enumerate(dense):                                 # ... and the pixels themselves
        assert want[0][d].tolist() == mc.dense_sums(m) + [0, 0], (what, d)


def test_mask_moments_on_the_host_cases_and_on_scanned_lists():
    small = [(vc.mask_to_rle_counts(m), m) for name, m in mc.host_masks() if m.shape == (5, 7)] + [mc.zero_length_runs()]
    check_mask_moments("5 x 7", [r for r, _ in small], [m for _, m in small], 5, 7)
    rs = np.random.RandomState(17)
    dense = [dict(mc.host_masks())["random"]]
    check_mask_moments("37 x 23", [vc.mask_to_rle_counts(dense[0])], dense, 37, 23)
    wide = rs.uniform(size=(H, W)) > 0.7
    wide[40:, 10], wide[:, 11:20], wide[:30, 20] = True, True, True      # one run over eleven columns, nine of them whole
    dense = [rs.uniform(size=(H, W)) > 0.5, vc.truth(0)["mask"], wide, vc.truth(1)["mask"]]
    lists = [vc.mask_to_rle_counts(m) for m in dense]
    assert len(lists[0]) > 4 * 256 and any(r > 3 * H for r in lists[2][1::2])       # more runs of ones than threads; runs over several whole columns
    check_mask_moments("96 x 128", lists, dense, H, W)


def test_mask_moments_of_the_largest_frame():
    for h, w in ((16384, 256), (256, 16384)):
        masks = scanned([[0, h * w], [h * w], [1, h * w - 2, 1]], h, w)
        mm, mstatus = maskfit.mask_moments(masks[0], h, w)
        want = ref.mask_moments(*masks[1], h, w)
        assert_bits(mm, want[0], f"{h} x {w}: mm")
        assert not mstatus.any().item() and want[0][0, 3] + want[0][0, 5] > 2 ** 48 and not want[0][1].any()
        assert (want[0][0] - want[0][2]).tolist() == [2, w - 1, h - 1, (w - 1) ** 2, (w - 1) * (h - 1), (h - 1) ** 2, 0, 0]


# ---------------------------------------------------------------------------------------------- 6. the step
def device_update(params=None):
    """maskfit.update behind maskfit_ref.update's signature; the device state travels in the dictionary."""
    def update(rows, status, mm, det, clipped, K, start, it, last, min_points, e, gain, poses, st, variant=None):
        n = len(poses)
        if "dev" not in st:
            st = dict(st, dev=maskfit.new_state(n, DEV), p32=_t(np.asarray(poses, np.float64).astype(np.float32)))
        best, score, state = st["dev"]
        poses_d = _t(np.asarray(poses, np.float64))
        maskfit.update(_t(rows), _t(np.asarray(status, np.int32)), _t(mm), _t(np.asarray(det, np.int32)), None if clipped is None else _t(np.asarray(clipped, np.int32)),
                       _t(np.asarray(K, np.float64)), _t(start), it, last, poses_d, st["p32"], best, score, state, min_points=min_points, min_elongation=e, gain=gain)
        new = dict(best=best.cpu().numpy(), score=score.cpu().numpy(), state=state.cpu().numpy(), dev=st["dev"], p32=st["p32"], p32_now=st["p32"].cpu().numpy())
        return poses_d.cpu().numpy(), st["p32"].cpu().numpy(), new
    return update


def test_update_on_the_planted_rows():
    p = mc.planted()
    want, got = mc.run_planted(p, ref.update), mc.run_planted(p, device_update())
    p32 = p["start"].astype(np.float32)
    for c, ((wp, ws), (gp, gs)) in enumerate(zip(want, got)):
        assert_bits(gp, wp, f"call {c}: poses")
        for k in ("best", "score", "state"):
            assert_bits(gs[k], ws[k], f"call {c}: {k}")
        touched = (want[c - 1][1]["state"][:, 0] & ref.STOP) == 0 if c else np.ones(len(wp), bool)
        p32[touched] = wp[touched].astype(np.float32)             # a pair that is stopped already is not touched
        assert_bits(gs["p32_now"], p32, f"call {c}: poses32")
    final = got[-1][1]["state"]
    assert final[:, 0].tolist() == p["want_bits"].tolist() and final[:, 1].tolist() == p["want_best"].tolist()
    bits = set(final[:, 0].tolist())
    assert {ref.FEW | ref.NOT_IMPROVED, ref.CLIPPED | ref.NOT_IMPROVED, ref.NO_MASK | ref.NOT_IMPROVED, ref.BAD_MASK | ref.NOT_IMPROVED, ref.ROUND, 0,
            ref.NOT_IMPROVED, ref.BAD_MASK | ref.CLIPPED | ref.NOT_IMPROVED, ref.ROUND | ref.NOT_IMPROVED} <= bits


def test_update_with_other_parameters_and_at_the_guards_of_the_turn():
    p = mc.planted()
    n = len(p["start"])
    rows, status, clipped = p["calls"][0]
    for min_points, e, gain in ((32, 0.1, 0.5), (1001, 0.1, 1.0), (1, 0.0, 0.25), (32, 0.45, 1.0)):
        want = ref.update(rows, status, p["mm"], p["det"], None, p["K"], p["start"], 0, False, min_points, e, gain, p["start"], ref.new_state(n))
        got = device_update()(rows, status, p["mm"], p["det"], None, p["K"], p["start"], 0, False, min_points, e, gain, p["start"], ref.new_state(n))
        assert_bits(got[0], want[0], f"{min_points} {e} {gain}: poses")
        assert_bits(got[1], want[1], "poses32")
        assert_bits(got[2]["state"], want[2]["state"], f"{min_points} {e} {gain}: state")
    tiny = 2.0 ** -10
    six = [mc.shape(4096, 64, 48, 4, 0, 16), mc.shape(4096, 64, 48, 4 - tiny, 0, 16), mc.shape(4096, 64, 48, 4, 4, 16), mc.shape(4096, 64, 48, 4, 4 + tiny, 16),
           mc.shape(4096, 64, 48, 4, -4, 16), mc.shape(4096, 64, 48, 4, -4 - tiny, 16), mc.shape(4096, 64, 48, -4, 0, 16), mc.shape(4096, 64, 48, 0, 4, 16)]
    rows = np.stack([mc.planted_row(s, 2000) for s in six])
    k = len(six)
    mm = np.asarray([mc.shape(4096, 72, 40, 4, 0, 16) + [0, 0], mc.shape(4096, 72, 40, 4 - tiny, 0, 16) + [0, 0]], np.int64)
    for det in (0, 1):
        args = (rows, np.zeros(k, np.int32), mm, np.full(k, det, np.int32), np.zeros(k, np.int32), np.tile(mc.EXACT_K, (k, 1)), np.tile(mc.exact_pose(), (k, 1, 1)), 0, False,
                32, 0.25, 1.0, np.tile(mc.exact_pose(), (k, 1, 1)), ref.new_state(k))
        want, got = ref.update(*args), device_update()(*args)
        assert_bits(got[0], want[0], "guards: poses")
        assert_bits(got[2]["state"], want[2]["state"], "guards: state")
        assert ((want[2]["state"][:, 0] & ref.ROUND) == 0).tolist() == ([True, False, True, False, True, False, False, False] if det == 0 else [False] * k)


# ---------------------------------------------------------------------------------------------- 7. MaskRefiner
def estimates_of(poses, scene, im, obj, instance):
    return [dict(scene_id=scene, im_id=im, obj_id=obj, score=0.9 - 0.01 * i, R=p[:3, :3].copy(), t=p[:3, 3].copy(), instance_id=instance)
            for i, p in enumerate(poses)]


KINDS = ("fit", "right", "wrong")


@functools.lru_cache(maxsize=None)
def scene():
    """The two instances on a frame each; per instance the fit starts, the right and the wrong hypotheses."""
    v, f = rc.mesh("boxes")
    models = {1: dict(vertices=v, faces=f, diameter=vc.SCALE)}
    cameras = {(1, i): dict(cam_K=mc.K) for i in range(2)}
    est = [e for i in range(2) for e in estimates_of(np.concatenate([mc.run(i, kind)[0] for kind in KINDS]), 1, i, 1, 10 + i)]
    masks = {10 + i: vc.segmentation(vc.truth(i)["runs"]) for i in range(2)}
    return models, cameras, est, masks


def check_fitted(out, est, what):
    want = {k: np.concatenate([mc.run(i, kind)[1][k] for i in range(2) for kind in KINDS]) for k in ("poses", "state", "score", "rows")}
    assert len(out) == len(est) == len(want["poses"])
    for i, (o, e) in enumerate(zip(out, est)):
        assert_bits(np.asarray(o["R"]), want["poses"][i, :3, :3], f"{what}: estimate {i}: R")
        assert_bits(np.asarray(o["t"]), want["poses"][i, :3, 3], f"{what}: estimate {i}: t")
        assert [o["maskfit_status"], o["best_iteration"]] == want["state"][i].tolist(), (what, i)
        assert_bits(o["iou_counts"], want["score"][i], f"{what}: estimate {i}: the IoUs as integers")
        assert_bits(o["moments"], want["rows"][i], f"{what}: estimate {i}: moments")
        s = want["score"][i].astype(np.float64)
        assert o["iou"] == s[0] / s[1] and o["iou_start"] == s[2] / s[3]
        assert all(o[k] == e[k] for k in ("scene_id", "im_id", "obj_id", "score", "instance_id"))
        if o["maskfit_status"] & ref.NOT_IMPROVED:
            assert_bits(np.asarray(o["R"]), np.asarray(e["R"]), "the input pose")
            assert_bits(np.asarray(o["t"]), np.asarray(e["t"]), "the input pose")


def test_refiner_equals_the_restatements_loop():
    models, cameras, est, masks = scene()
    check_fitted(maskfit.MaskRefiner(models, cameras).refine(est, masks), est, "one chunk")
    check_fitted(maskfit.MaskRefiner(models, cameras, pairs_per_call=2).refine(est, masks), est, "chunks of 2")
    per_estimate = [masks[e["instance_id"]] for e in est]
    sized = {k: dict(c, size=(H, W)) for k, c in cameras.items()}
    check_fitted(maskfit.MaskRefiner(models, sized).refine(est, per_estimate), est, "one mask per estimate")
    none = maskfit.MaskRefiner(models, cameras).refine(est[:3], [None, masks[10], None])
    assert [o["maskfit_status"] for o in none[::2]] == [ref.NO_MASK | ref.NOT_IMPROVED] * 2 and none[1]["best_iteration"] > 0
    assert_bits(np.asarray(none[0]["R"]), np.asarray(est[0]["R"]), "no mask: the input pose")


def test_fit_refine_and_select():
    from gigapose_amd import refine, verify

    v, f = rc.mesh("boxes")
    models = {1: dict(vertices=v, faces=f, diameter=vc.SCALE)}
    cameras = {(1, 0): dict(cam_K=mc.K, depth=vc.truth(0)["depth"])}
    p, host = mc.run(0, "stage")
    est = [dict(e, instance_id=20 + i) for i, e in enumerate(estimates_of(p, 1, 0, 1, 0))]
    masks = {20 + i: vc.segmentation(vc.truth(0)["runs"]) for i in range(len(est))}
    fitter = maskfit.MaskRefiner(models, cameras)
    refiner = refine.DepthRefiner(models, cameras, iters=rc.ITERS, box="frame")
    chosen = maskfit.fit_refine_and_select(fitter, refiner, verify.HypothesisVerifier(models, cameras), est, masks)
    want = mc.depth_refined(host["poses"])
    assert [e["instance_id"] for e in chosen] == [20, 21, 22, 23]
    alone = refiner.refine(est)
    for i, e in enumerate(chosen):
        assert_bits(np.asarray(e["R"]), want[i, :3, :3], f"start {i}: R")
        assert_bits(np.asarray(e["t"]), want[i, :3, 3], f"start {i}: t")
        start = rc.deviation(v, p[i], rc.GT)
        assert rc.deviation(v, rc.rigid(e["R"], e["t"]), rc.GT) < 0.01 * start < 0.02 * rc.deviation(v, rc.rigid(alone[i]["R"], alone[i]["t"]), rc.GT)
    # RGB only: no depth, no refiner; three wrong hypotheses first
    models, rgb, _, _ = scene()
    est = estimates_of(vc.hypotheses(0), 1, 0, 1, 10) + estimates_of(vc.hypotheses(1), 1, 1, 1, 11)
    masks = {10 + i: vc.segmentation(vc.truth(i)["runs"]) for i in range(2)}
    chosen = maskfit.fit_refine_and_select(maskfit.MaskRefiner(models, rgb), None, verify.HypothesisVerifier(models, rgb), est, masks)
    assert [e["instance_id"] for e in chosen] == [10, 11]
    for which, e in enumerate(chosen):
        k = round((0.9 - e["score"]) / 0.01)
        assert k >= 3 and e["score"] == est[6 * which + k]["score"] and e["iou"] > 0.75
