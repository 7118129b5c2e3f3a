"""CPU: the host half of the ground-truth visibility stage (gigapose_amd/gtinfo.py, libgigapose_gtinfo.so,
include/gigapose_gtinfo.h) and of the scorers' min_visib.

The numpy restatement of the header (gigapose_testing/gtinfo_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_gtinfo.py); here it is held to things that cannot share its mistakes: a pixel-by-pixel reading in Python sets and
Python numbers over planted keys, depths and rays on which every comparison is exact; ingest.mask_to_rle_counts and numpy's prefix
sums for the run lists, and the decoders' parity rule for the way back; and what the numbers are for -- on the scene of
refine_cases (the three-box object, 96 x 128) an object nothing hides is wholly visible, with delta = 0 a pixel is visible for
exactly the instances that attain the z-buffer's minimum, an object behind another loses exactly the overlapped pixels, one that
leaves the frame loses the part outside (which is what the canvas is for), a wall hides everything.  Eight subtly wrong versions
fail these checks.  Beside that: min_visib against brute-force matching, the library against its header, and every refusal of the
limits, which needs no device."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, distances, evaluate, gtinfo
from gigapose_amd.ingest import mask_to_rle_counts
from gigapose_testing import gtinfo_cases as cases
from gigapose_testing import gtinfo_ref, raster_ref
from gigapose_testing.symbols import exported_symbols

INF = float("inf")


# ---------------------------------------------------------------------------------------------- an independent reading
def f32_of(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def read_in_sets(keys, origin, depth, ray, delta, H, W):
    """One instance pixel by pixel, in Python numbers -> the sets of FRAME coordinates (x, y): object pixels of the canvas, those in
    the frame, the measured ones, the visible ones.  depth None: no image."""
    ox, oy = origin
    everywhere, inside, valid, visible = set(), set(), set(), set()
    for cy, row in enumerate(keys):
        for cx, key in enumerate(row):
            if key == 2 ** 64 - 1:
                continue
            dm = f32_of(key >> 32)
            if not 0 < dm < INF:                                      # false for a NaN
                continue
            x, y = cx - ox, cy - oy
            everywhere.add((x, y))
            if not (0 <= x < W and 0 <= y < H):
                continue
            inside.add((x, y))
            dt = 0.0 if depth is None else float(depth[y][x])
            if not 0 < dt < INF:
                dt = 0.0
            if dt > 0:
                valid.add((x, y))
            r = float(ray[y][x])
            if dt == 0 or dm * r - dt * r <= delta:
                visible.add((x, y))
    return everywhere, inside, valid, visible


def box_of(points):
    return list(gtinfo_ref.BOX_EMPTY) if not points else [min(p[0] for p in points), min(p[1] for p in points), max(p[0] for p in points),
                                                          max(p[1] for p in points)]


def reading_agrees(case, variant=None, with_depth=True):
    """Does the restatement (or a wrong variant) give, for every instance of a planted case, what the sets give?"""
    H, W = case["H"], case["W"]
    args = cases.call(case) if with_depth else cases.call(case, depth=None)
    vis, origin, depth, frame, ray, ray_index, delta = args
    cls, info, box, status = gtinfo_ref.classify(*args, variant=variant)
    if status.any() or cls.shape != (len(vis), W, H):
        return False
    ok = True
    for n in range(len(vis)):
        d = None if depth is None else depth[frame[n]].tolist()
        everywhere, inside, valid, visible = read_in_sets(vis[n].tolist(), origin, d, ray[ray_index[n]].tolist(), delta, H, W)
        ok = ok and info[n].tolist() == [len(everywhere), len(inside), len(valid), len(visible)]
        ok = ok and box[n].tolist() == box_of(everywhere) + box_of(visible)
        got = cls[n].tolist()                                          # [x][y]: column-major
        ok = ok and {(x, y) for x in range(W) for y in range(H) if got[x][y] & 1} == inside
        ok = ok and {(x, y) for x in range(W) for y in range(H) if got[x][y] & 2} == visible
        ok = ok and all(v in (0, 1, 3) for col in got for v in col)
    return ok


@functools.lru_cache(maxsize=None)
def planted_cases():
    return [cases.planted_case(H, W, canvas, origin, seed) for seed, (H, W) in enumerate(cases.FRAMES) for canvas, origin in cases.origins(H, W)]


def planted_hold_what_they_say():
    """The planted pixels, read in sets, are what their names say -- a check of the cases, not of the restatement."""
    for case in planted_cases():
        vis, origin, depth, frame, ray, ray_index, delta = cases.call(case)
        for n, (obj, seen, measured) in enumerate(case["expect"]):
            sets = read_in_sets(vis[n].tolist(), origin, depth[frame[n]].tolist(), ray[ray_index[n]].tolist(), delta, case["H"], case["W"])
            assert [len(s) for s in sets] == [obj, obj, obj * measured, seen], (case["names"][n], case["H"], case["W"])


def test_planted_pixels_hold_every_branch_of_the_rule():
    planted_hold_what_they_say()
    kinds = cases.planted_pixels()
    names = [k[0] for k in kinds]
    for needed in ("not covered", "dm = 0", "dm < 0", "dm NaN", "dm +inf", "dt = 0", "dt < 0", "dt NaN", "dt +inf", "Dm - Dt exactly delta",
                   "one step above delta"):
        assert needed in names
    at, above = kinds[names.index("Dm - Dt exactly delta")], kinds[names.index("one step above delta")]
    for (_, key, dt, r, _, _, _), want in ((at, cases.DELTA), (above, float(np.nextafter(cases.DELTA, INF)))):
        dm = f32_of(int(key) >> 32)
        assert dm * r - float(dt) * r == want and float(dt) > 0                    # exactly delta; exactly one float64 step above it


def test_restatement_equals_the_set_reading_on_planted_pixels_frames_and_canvases():
    """Frames 1 x 1, 1 x W, H x 1, 37 x 23, 65 x 63, each on the frame itself (ox = oy = 0), on margin 1.0 and on an odd canvas; object
    pixels only outside the frame, only inside, on the four frame edges from both sides, on the canvas' corners and edges."""
    seen = set()
    for case in planted_cases():
        assert reading_agrees(case), (case["H"], case["W"], case["args"]["origin"])
        assert reading_agrees(case, with_depth=False), ("no depth", case["H"], case["W"])
        seen.add((case["H"], case["W"], case["args"]["origin"] == (0, 0)))
        assert {"only outside", "only inside", "frame edges", "canvas edges"} <= set(case["names"])
    assert {(h, w, True) for h, w in cases.FRAMES} <= seen and {(h, w, False) for h, w in cases.FRAMES} <= seen


def test_restatement_marks_bad_pairs_and_leaves_their_rows_initial():
    case = planted_cases()[4]
    vis, origin, depth, frame, ray, ray_index, delta = cases.call(case)
    frame, ray_index = frame.copy(), ray_index.copy()
    frame[1], ray_index[2], frame[3], ray_index[3] = len(depth), -1, -1, len(ray)
    cls, info, box, status = gtinfo_ref.classify(vis, origin, depth, frame, ray, ray_index, delta)
    assert status[:5].tolist() == [0, gtinfo_ref.BAD_FRAME, gtinfo_ref.BAD_RAY, gtinfo_ref.BAD_FRAME | gtinfo_ref.BAD_RAY, 0]
    for n in (1, 2, 3):
        assert not cls[n].any() and not info[n].any() and box[n].tolist() == list(gtinfo_ref.BOX_EMPTY) * 2
    _, _, _, status = gtinfo_ref.classify(vis, origin, None, frame, ray, ray_index, delta)      # without depth the frame is not read
    assert status[:5].tolist() == [0, 0, gtinfo_ref.BAD_RAY, gtinfo_ref.BAD_RAY, 0]


# ---------------------------------------------------------------------------------------------- the run lists
def rank_parity(cum, p):
    """gp_key_walk.h's rank_of by bisection over a Python list, then its parity: the mask value of column-major pixel p."""
    a, b = 0, len(cum)
    while a < b:
        mid = a + ((b - a) >> 1)
        if cum[mid] <= p:
            a = mid + 1
        else:
            b = mid
    return a & 1


def run_lists_agree(variant=None, chunk=8):
    """Every mask as the object bit and its complement-free copy as the visible bit, small chunks so that several fall into a mask."""
    masks = cases.run_masks()
    ok = True
    for name, mask in masks:
        h, w = mask.shape
        cls = cases.cls_of(mask[None])
        for which in (0, 1):
            counts, cum, offsets = gtinfo_ref.encode_runs(cls, which, variant, chunk)
            want = mask_to_rle_counts(mask)
            ok = ok and offsets.tolist() == [0, len(want)] and counts.tolist() == want.tolist() and cum.tolist() == np.cumsum(want).tolist()
            if len(cum) and ok:
                ok = ok and [[rank_parity(cum.tolist(), x * h + y) for x in range(w)] for y in range(h)] == mask.astype(int).tolist()
    return ok


def test_run_lists_equal_the_ingest_encoder_and_decode_back():
    assert run_lists_agree()
    assert run_lists_agree(chunk=gtinfo_ref.CHUNK)
    names = [n for n, _ in cases.run_masks()]
    assert len(names) >= len(cases.mc.host_masks()) + 6
    board = dict(cases.run_masks())["checkerboard from pixel 0"]
    counts, _, _ = gtinfo_ref.encode_runs(cases.cls_of(board[None]), 0)
    assert len(counts) == board.size + 1 and counts[0] == 0                       # H*W + 1 entries: the first run is zeros, of length 0
    three = dict(cases.run_masks())["one run across three columns"]
    assert gtinfo_ref.encode_runs(cases.cls_of(three[None]), 0)[0].tolist() == [13, 9, 13]
    for name, mask in cases.run_masks():                                         # the two bits of one cls are encoded independently
        other = np.roll(mask, 1, axis=1) & mask
        cls = cases.cls_of(mask[None], other[None])
        assert gtinfo_ref.encode_runs(cls, 0)[0].tolist() == mask_to_rle_counts(mask).tolist(), name
        assert gtinfo_ref.encode_runs(cls, 1)[0].tolist() == mask_to_rle_counts(other).tolist(), name
        assert (gtinfo_ref.decode(gtinfo_ref.encode_runs(cls, 1)[1], *mask.shape) == other).all(), name


def test_a_slice_of_the_wrong_length_writes_nothing_and_reports_the_instance():
    masks = [m for _, m in cases.run_masks() if m.shape == (5, 7)][:4]
    cls = cases.cls_of(np.stack(masks))
    counts, cum, offsets = gtinfo_ref.encode_runs(cls, 0)
    for bad in ("short", "long", "inverted", "beyond"):
        off = offsets.astype(np.int64).copy()
        total = int(off[-1]) + 3
        if bad == "short":
            off[2:] += 1                                                         # instance 1 gets one entry more than it has runs ...
            off[3:] -= 1                                                         # ... and instance 2 one fewer
            want_err, spared = (2, 3), (0, 3)
        elif bad == "long":
            off[3:] += 2
            want_err, spared = (3,), (0, 1, 3)
        elif bad == "inverted":
            off[1] = -1
            want_err, spared = (1, 2), (2, 3)
        else:
            off[-1] = total + 1
            want_err, spared = (4,), (0, 1, 2)
        out_counts, out_cum = np.full(total, -7, np.int32), np.full(total, -7, np.int32)
        err = gtinfo_ref.write_runs(cls, 0, off, out_counts, out_cum)
        assert err in want_err, bad
        written = np.zeros(total, bool)
        for n in spared:
            lo, hi = int(off[n]), int(off[n + 1])
            assert out_counts[lo:hi].tolist() == counts[offsets[n]:offsets[n + 1]].tolist(), (bad, n)
            assert out_cum[lo:hi].tolist() == cum[offsets[n]:offsets[n + 1]].tolist(), (bad, n)
            written[lo:hi] = True
        assert (out_counts[~written] == -7).all() and (out_cum[~written] == -7).all(), bad      # nothing else is touched


# ---------------------------------------------------------------------------------------------- what the numbers are for
def object_mask(name, margin=1.0):
    return cases.drawn(name, margin) != raster_ref.EMPTY_KEY


@functools.lru_cache(maxsize=None)
def checks(variant=None):
    """-> {name: passed} for the restatement or a wrong variant of it."""
    out = {}
    out["planted"] = all(reading_agrees(c, variant) for c in planted_cases()[6:12])            # 7 x 1 and 37 x 23 on their three canvases
    out["runs"] = run_lists_agree(variant)
    models, cameras, gts = cases.scene()
    names = [n for n, _ in cases.SCENE]
    rows = gtinfo_ref.compute(models, cameras, gts, delta=15.0, margin=1.0, masks=True, variant=variant)[(1, 1)]
    by = dict(zip(names, rows))
    front, behind = cases.window(object_mask("front")), cases.window(object_mask("behind"))
    # an object nothing hides
    out["free"] = by["free"]["visib_fract"] == 1 and by["front"]["visib_fract"] == 1 and by["free"]["px_count_visib"] == int(object_mask("free").sum())
    # an object behind another loses exactly the overlapped pixels
    seen = gtinfo_ref.decode(np.cumsum(by["behind"]["mask_visib"]["counts"]), cases.H, cases.W) if sum(by["behind"]["mask_visib"]["counts"]) == cases.H * cases.W else None
    out["behind"] = seen is not None and (seen == (behind & ~front)).all() and 0 < (behind & front).sum() < behind.sum() \
        and by["behind"]["px_count_visib"] == int((behind & ~front).sum()) and by["behind"]["px_count_all"] == int(behind.sum())
    amodal = gtinfo_ref.decode(np.cumsum(by["behind"]["mask"]["counts"]), cases.H, cases.W) if sum(by["behind"]["mask"]["counts"]) == cases.H * cases.W else None
    out["behind"] = out["behind"] and amodal is not None and (amodal == behind).all()
    # delta = 0: visible for exactly the instances that attain the minimum
    rows0 = gtinfo_ref.compute(models, cameras, gts, delta=0.0, margin=1.0, masks=True, variant=variant)[(1, 1)]
    z = cases.z_buffer()
    ok = True
    for name, row in zip(names, rows0):
        keys = cases.window(cases.drawn(name))
        attains = (keys != raster_ref.EMPTY_KEY) & (gtinfo_ref.key_depth(keys) == z)
        ok = ok and (((row["cls"].T & 2) != 0) == attains).all()
    covered = np.stack([cases.window(object_mask(n)) for n in names]).any(axis=0)
    ok = ok and (np.stack([(r["cls"].T & 2) != 0 for r in rows0]).any(axis=0) == covered).all()      # somebody is visible wherever anything is drawn
    out["minimum"] = ok
    # half out of the frame: the in-frame share at margin 1.0, 1 at margin 0; the amodal box leaves the frame
    m1, c1, g1 = cases.scene(np.zeros((cases.H, cases.W), np.float32), ("half out",))
    wide = gtinfo_ref.compute(m1, c1, g1, margin=1.0, variant=variant)[(1, 1)][0]
    tight = gtinfo_ref.compute(m1, c1, g1, margin=0.0, variant=variant)[(1, 1)][0]
    whole, shown = object_mask("half out"), cases.window(object_mask("half out"))
    out["half out"] = (0 < shown.sum() < whole.sum() and wide["px_count_all"] == int(whole.sum()) and wide["px_count_visib"] == int(shown.sum())
                       and wide["visib_fract"] == int(shown.sum()) / int(whole.sum()) and tight["visib_fract"] == 1
                       and wide["bbox_obj"][0] < 0 and tight["bbox_obj"][0] == 0 and wide["bbox_visib"][0] == 0
                       and wide["bbox_obj"][0] + wide["bbox_obj"][2] == wide["bbox_visib"][0] + wide["bbox_visib"][2])
    # a wall in front of everything
    wall = np.full((cases.H, cases.W), 100.0, np.float32)
    hidden = gtinfo_ref.compute(*cases.scene(wall), variant=variant)[(1, 1)]
    out["wall"] = all(r["px_count_visib"] == 0 and r["bbox_visib"] == [-1, -1, -1, -1] and r["visib_fract"] == 0 and r["px_count_valid"] == r["px_count_all"] > 0
                      and r["bbox_obj"][2] > 0 for r in hidden)
    # no measurement anywhere: everything drawn in the frame is visible, nothing is valid
    blind = gtinfo_ref.compute(*cases.scene(np.zeros((cases.H, cases.W), np.float32)), variant=variant)[(1, 1)]
    out["blind"] = all(r["visib_fract"] == 1 and r["px_count_valid"] == 0 for r in blind)
    return out


def test_the_scene_checks_hold_for_the_restatement():
    out = checks()
    assert all(out.values()), out


@pytest.mark.parametrize("variant", gtinfo_ref.VARIANTS)
def test_the_checks_reject_wrong_versions(variant):
    """Row-major flattening; < for <= at delta; z-depth in place of the ray distance (the decisive planted pixel lies off the
    principal axis); px_count_all from the frame only; dt == 0 not visible; the first run taken as ones; the last entry missing; a
    chunk's first pixel compared with 0 in place of the previous chunk's last pixel."""
    must_fail = {"row_major": ("planted", "behind"), "strict_delta": ("planted",), "z_depth": ("planted",), "all_from_frame": ("planted", "half out"),
                 "unmeasured_hidden": ("planted", "blind"), "first_run_ones": ("runs",), "last_missing": ("runs",), "chunk_start_zero": ("runs",)}[variant]
    out = checks(variant)
    for name in must_fail:
        assert not out[name], name


# ---------------------------------------------------------------------------------------------- min_visib
def brute_force_counted(errors, threshold, valid):
    """The rule read literally: estimates in the given (descending score) order; each looks at every ground truth nobody has taken --
    visible or not --, picks the one with the smallest error and takes it if that error is below the threshold; only the taken ground
    truths that are valid are counted."""
    taken = []
    for row in errors:
        best = None
        for g, err in enumerate(row):
            if g in taken:
                continue
            if best is None or err < row[best]:
                best = g
        if best is not None and row[best] < threshold:
            taken.append(best)
    return sum(1 for g in taken if valid[g])


def small_scene_errors():
    """The hand-made error tables of tests/test_eval_host.py's recall test (same seed, same shapes)."""
    rs = np.random.RandomState(9)
    T = 10
    per_target = []
    for obj, E, G in ((1, 3, 2), (2, 1, 1), (1, 0, 2), (2, 2, 0)):
        per_target.append((dict(obj_id=obj), dict(mssd=rs.uniform(0, 60, (E, G)), mspd=rs.uniform(0, 120, (E, G)),
                                                  vsd=np.round(rs.uniform(0, 1, (E, G, T)), 2), clipped=np.zeros((E, G), bool))))
    return per_target, {1: 100.0, 2: 60.0}


def test_match_greedy_counts_only_the_valid_and_keeps_its_default():
    rs = np.random.RandomState(6)
    for _ in range(300):
        E, G = rs.randint(0, 5), rs.randint(0, 4)
        errors = np.round(rs.uniform(0, 1, (E, G)), 1)
        valid = rs.uniform(size=G) < 0.6
        for th in (0.25, 0.5, 0.75):
            assert evaluate.match_greedy(errors, th) == brute_force_counted(errors.tolist(), th, [True] * G)
            got = evaluate.match_greedy(errors, th, valid)
            assert type(got) is int and got == brute_force_counted(errors.tolist(), th, valid.tolist())
    # an estimate that lands on the hidden ground truth is not free to take a visible one too
    errors = np.asarray([[0.1, 0.2]])
    assert evaluate.match_greedy(errors, 0.5, [False, True]) == 0 and evaluate.match_greedy(errors, 0.5, [True, False]) == 1
    assert evaluate.match_greedy(np.asarray([[0.1, 0.2], [0.15, 0.3]]), 0.5, [False, True]) == 1       # the second estimate takes the visible one


def test_min_visib_none_reproduces_the_present_recalls_and_a_hidden_ground_truth_changes_neither_count():
    per_target, diam = small_scene_errors()
    base = evaluate.recall_from_errors(per_target, diam, W=1280)
    assert evaluate.recall_from_errors(per_target, diam, W=1280, min_visib=None) == base and base["targets"] == 5
    for i in range(10):
        want = sum(brute_force_counted(e["mssd"].tolist(), evaluate.CORRECT_THS[i] * diam[t["obj_id"]], [True] * e["mssd"].shape[1]) for t, e in per_target) / 5
        assert base["recall_mssd"][i] == want
    # every ground truth visible: min_visib changes nothing
    seen = [(t, dict(e, visib=np.ones(e["mssd"].shape[1]))) for t, e in per_target]
    assert evaluate.recall_from_errors(seen, diam, W=1280, min_visib=0.1) == base
    # a hidden ground truth added to every target, far from every estimate: numerator and denominator stay
    def with_hidden(e, err):
        E, G = e["mssd"].shape
        far = {k: np.concatenate([e[k], np.full((E, 1) + e[k].shape[2:], v)], axis=1) for k, v in (("mssd", err), ("mspd", err), ("vsd", min(err, 1.0)))}
        return dict(far, clipped=np.zeros((E, G + 1), bool), visib=np.concatenate([np.ones(G), [0.05]]))

    hidden = [(t, with_hidden(e, 1e9)) for t, e in per_target]
    assert evaluate.recall_from_errors(hidden, diam, W=1280, min_visib=0.1) == base
    counted_all = evaluate.recall_from_errors(hidden, diam, W=1280)                                 # without the filter the denominator grows
    assert counted_all["targets"] == 9 and counted_all["ar"] < base["ar"]
    # a hidden ground truth ON which the estimates land (error 0): it absorbs them, so the recalls can only fall, and they equal the brute force
    absorbing = [(t, with_hidden(e, 0.0)) for t, e in per_target]
    out = evaluate.recall_from_errors(absorbing, diam, W=1280, min_visib=0.1)
    assert out["targets"] == 5 and out["ar"] < base["ar"]
    for i in range(10):
        want = sum(brute_force_counted(e["mssd"].tolist(), evaluate.CORRECT_THS[i] * diam[t["obj_id"]], (e["visib"] >= 0.1).tolist()) for t, e in absorbing) / 5
        assert out["recall_mssd"][i] == want
        want = sum(brute_force_counted(e["mspd"].tolist(), 5.0 * (i + 1) * 2.0, (e["visib"] >= 0.1).tolist()) for t, e in absorbing) / 5
        assert out["recall_mspd"][i] == want
        for k in range(10):
            want = sum(brute_force_counted(e["vsd"][:, :, k].tolist(), evaluate.CORRECT_THS[i], (e["visib"] >= 0.1).tolist()) for t, e in absorbing) / 5
            assert out["recall_vsd"][k][i] == want
    # the threshold itself counts: visib_fract == min_visib is visible
    edge = [(t, dict(e, visib=np.full(e["mssd"].shape[1], 0.1))) for t, e in per_target]
    assert evaluate.recall_from_errors(edge, diam, W=1280, min_visib=0.1) == base


def test_scorers_take_min_visib_and_refuse_ground_truths_without_the_key():
    mesh = dict(vertices=np.zeros((3, 3), np.float32), faces=np.zeros((1, 3), np.int32), diameter=100.0)
    cams = {(1, 1): dict(cam_K=[500.0, 0, 32, 0, 500.0, 24, 0, 0, 1], depth=np.zeros((48, 64), np.float32))}
    targets = [dict(scene_id=1, im_id=1, obj_id=1, inst_count=1)]
    gt = dict(obj_id=1, cam_R_m2c=np.eye(3).reshape(-1), cam_t_m2c=[0, 0, 1])
    est = [dict(scene_id=1, im_id=1, obj_id=1, score=0.5, R=np.eye(3), t=np.asarray([0.0, 0.0, 1.0]))]
    for make in (lambda g, **kw: evaluate.PoseScorer({1: mesh}, targets, g, cams, **kw), lambda g, **kw: distances.AddScorer({1: mesh}, targets, g, **kw)):
        assert make({(1, 1): [gt]}).min_visib is None and make({(1, 1): [gt]}, min_visib=0.1).min_visib == 0.1
        with pytest.raises(ValueError, match="visib_fract"):
            make({(1, 1): [gt]}, min_visib=0.1).errors(est)                     # before any GPU work
        for bad in (-0.1, 1.5):
            with pytest.raises(ValueError, match="min_visib"):
                make({(1, 1): [gt]}, min_visib=bad)
    # the ADD recalls: the same rule through recall_from_add_errors
    rs = np.random.RandomState(2)
    per_target = [(dict(obj_id=1), dict(add=rs.uniform(0, 30, (3, 3)), adds=rs.uniform(0, 30, (3, 3)), visib=np.asarray([1.0, 0.05, 0.5])))]
    out = distances.recall_from_add_errors(per_target, {1: 100.0}, {1: False}, min_visib=0.1)
    assert out["targets"] == 2
    assert out["recall_add"] == brute_force_counted(per_target[0][1]["add"].tolist(), 10.0, [True, False, True]) / 2
    plain = distances.recall_from_add_errors([(t, {k: v for k, v in e.items() if k != "visib"}) for t, e in per_target], {1: 100.0}, {1: False})
    assert plain["targets"] == 3 and plain["recall_add"] == brute_force_counted(per_target[0][1]["add"].tolist(), 10.0, [True] * 3) / 3


def test_with_visibility_adds_the_key_to_copies():
    gts = {(1, 1): [dict(obj_id=1, cam_R_m2c=[1] * 9, cam_t_m2c=[0, 0, 1]), dict(obj_id=2, cam_R_m2c=[1] * 9, cam_t_m2c=[0, 0, 2])], (1, 2): []}
    info = {(1, 1): [dict(visib_fract=0.25), dict(visib_fract=0.0)], (1, 2): []}
    out = gtinfo.with_visibility(gts, info)
    assert [g["visib_fract"] for g in out[(1, 1)]] == [0.25, 0.0] and out[(1, 2)] == [] and "visib_fract" not in gts[(1, 1)][0]
    assert out[(1, 1)][1]["cam_t_m2c"] == [0, 0, 2]
    with pytest.raises(ValueError, match="lists 2"):
        gtinfo.with_visibility(gts, {(1, 1): [dict(visib_fract=1.0)], (1, 2): []})


def test_device_masks_assign_what_pack_masks_works_out():
    from gigapose_amd import hypotheses

    i32 = torch.int32
    lists = (torch.tensor([3, 35, 35], dtype=i32), torch.tensor([0, 2, 3], dtype=i32))
    masks = hypotheses.DeviceMasks(lists, [32, 0], [[0, 0, 6, 4], [7, 5, -1, -1]], (5, 7))
    table = hypotheses.CameraTable("test", {(1, 1): dict(cam_K=cases.K)}, "ignored")
    est = [dict(instance_id=1), dict(instance_id=0), dict(instance_id=7)]
    det, area, boxes = masks.assign("test", est, table)
    assert det.tolist() == [1, 0, -1] and area[:2].tolist() == [0.0, 32.0] and np.isnan(area[2]) and boxes.shape == (2, 4)
    assert (table.H, table.W) == (5, 7) and masks.lists[0] is lists[0]
    with pytest.raises(ValueError, match="instance_id"):
        masks.assign("test", [dict()], table)
    with pytest.raises(ValueError, match="frame sizes differ"):
        masks.assign("test", est, hypotheses.CameraTable("test", {(1, 1): dict(cam_K=cases.K, size=(5, 8))}, "ignored"))
    with pytest.raises(ValueError, match="offsets"):
        hypotheses.DeviceMasks((lists[0], lists[1].long()), [1], [[0, 0, 0, 0]], (5, 7))
    named = hypotheses.DeviceMasks(lists, [32, 0], [[0, 0, 6, 4], [7, 5, -1, -1]], (5, 7), index={"a": 1})
    assert named.assign("test", [dict(instance_id="a"), dict(instance_id=1)], table)[0].tolist() == [1, -1]


# ---------------------------------------------------------------------------------------------- the library and its header
def test_gtinfo_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_gtinfo.so", "gpg")       # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_gtinfo.h" and side.path == gtinfo.GTINFO_LIB_PATH
    assert sorted(protos) == ["gpg_abi_version", "gpg_classify", "gpg_count_runs", "gpg_last_error", "gpg_pixels_per_workgroup",
                              "gpg_runs_workspace_bytes", "gpg_write_runs"]
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpg_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_", "gpf_", "gpv_", "gpm_", "gpl_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the gtinfo library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert lib.gpg_last_error.restype is ctypes.c_char_p
    assert list(lib.gpg_classify.argtypes) == [P, I, I, I, I, P, I, P, P, I, P, D, I, I, I, P, P, P, P, P]
    assert list(lib.gpg_count_runs.argtypes) == [P, I, I, I, I, P, P, P]
    assert list(lib.gpg_write_runs.argtypes) == [P, I, I, I, I, P, P, I, P, P, P, P]
    assert lib.gpg_runs_workspace_bytes.restype is ctypes.c_size_t and list(lib.gpg_runs_workspace_bytes.argtypes) == [I, I, I]      # sizes are size_t
    assert lib.gpg_abi_version() >= 1
    C = lib.gpg_pixels_per_workgroup()
    assert C == gtinfo.pixels_per_workgroup() == gtinfo_ref.CHUNK and C % 64 == 0 and 2 * C + 1 <= 96 * 128
    assert lib.gpg_runs_workspace_bytes(3, 96, 128) == 3 * 3 * 8 and lib.gpg_runs_workspace_bytes(1, 1, C + 1) == 16
    assert lib.gpg_runs_workspace_bytes(65535, 2048, 2048) == 65535 * 1024 * 8                                  # the largest: 1 024 chunks each
    for bad in ((-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 2048, 2049)):
        assert lib.gpg_runs_workspace_bytes(*bad) == 0
    for name in ("INFO", "BOX", "PX_ALL", "PX_FRAME", "PX_VALID", "PX_VISIB", "CLS_OBJECT", "CLS_VISIBLE", "BAD_FRAME", "BAD_RAY"):
        assert getattr(gtinfo_ref, name) == getattr(gtinfo, name), name
    assert gtinfo_ref.BOX_EMPTY == (gtinfo.BOX_EMPTY_MIN, gtinfo.BOX_EMPTY_MIN, gtinfo.BOX_EMPTY_MAX, gtinfo.BOX_EMPTY_MAX)
    header = open(_lib.INCLUDE_DIR + "/gigapose_gtinfo.h").read()
    for name, value in (("GPG_INFO", 4), ("GPG_BOX", 8), ("GPG_PX_ALL", 0), ("GPG_PX_FRAME", 1), ("GPG_PX_VALID", 2), ("GPG_PX_VISIB", 3),
                        ("GPG_CLS_OBJECT", 1), ("GPG_CLS_VISIBLE", 2), ("GPG_BAD_FRAME", 1), ("GPG_BAD_RAY", 2),
                        ("GPG_BOX_EMPTY_MIN", 2 ** 30), ("GPG_BOX_EMPTY_MAX", -2 ** 30)):
        assert f"#define {name} {value}" in header and getattr(gtinfo, name[4:]) == value, name


def test_gtinfo_argument_validation_of_the_library_needs_no_gpu():
    lib = gtinfo.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    err = lib.gpg_last_error
    names = ["vis", "depth", "frame", "ray", "ray_index", "cls", "info", "box", "status"]

    def classify(Hc=288, Wc=384, ox=128, oy=96, M=1, R=1, delta=15.0, N=3, H=96, W=128, **ptrs):
        p = {k: ptrs.get(k, one) for k in names}
        return lib.gpg_classify(p["vis"], Hc, Wc, ox, oy, p["depth"], M, p["frame"], p["ray"], R, p["ray_index"], delta, N, H, W, p["cls"], p["info"],
                                p["box"], p["status"], null)

    # every limit of the header, each with its message.  Nothing is launched on this machine: the calls that pass are the N = 0 ones
    for kw, msg in ((dict(N=-1), b"instances"), (dict(N=65536), b"instances"),
                    (dict(H=0), b"bad frame"), (dict(W=0), b"bad frame"), (dict(H=2048, W=2049, Hc=4096, Wc=4096, ox=0, oy=0), b"bad frame"),
                    (dict(Hc=0), b"bad canvas"), (dict(Wc=-1), b"bad canvas"), (dict(Hc=32768, Wc=65536), b"bad canvas"), (dict(Hc=46341, Wc=46341), b"bad canvas"),
                    (dict(Hc=1, Wc=2 ** 30 + 1, H=1, W=1, ox=0, oy=0), b"bad canvas"),
                    (dict(ox=-1), b"leaves the canvas"), (dict(oy=-1), b"leaves the canvas"), (dict(ox=257), b"leaves the canvas"), (dict(oy=193), b"leaves the canvas"),
                    (dict(ox=2 ** 31 - 1), b"leaves the canvas"),
                    (dict(M=0), b"bad sizes"), (dict(R=0), b"bad sizes"), (dict(delta=float("nan")), b"NaN")):
        assert classify(**kw) == -1 and b"gpg_classify" in err() and msg in err(), (kw, err())
    for name in ("vis", "ray", "ray_index", "cls", "info", "box", "status", "frame"):     # each required pointer in turn
        assert classify(**{name: null}) == -1 and b"null" in err(), name
    assert classify(info=ctypes.c_void_p(12)) == -1 and b"aligned" in err()
    assert classify(vis=ctypes.c_void_p(12)) == -1 and b"aligned" in err()
    everything = {k: null for k in names}
    assert classify(N=0, **everything) == 0 and classify(N=0, H=0, **everything) == -1 and b"bad frame" in err()     # N = 0: the sizes are still checked
    assert classify(N=0, M=0, **everything) == 0 and classify(N=0, M=0, **dict(everything, depth=one)) == -1         # M belongs to depth
    assert classify(N=0, Hc=96, Wc=128, ox=0, oy=0, **everything) == 0                                               # the canvas may be the frame
    assert classify(N=0, Hc=46340, Wc=46340, **everything) == 0 and classify(N=0, ox=256, oy=192, **everything) == 0  # the largest that pass

    def count(N=3, H=96, W=128, which=0, cls=one, runs=one, work=one):
        return lib.gpg_count_runs(cls, N, H, W, which, runs, work, null)

    def write(N=3, H=96, W=128, which=0, total=10, cls=one, work=one, offsets=one, counts=one, cum=one, e=one):
        return lib.gpg_write_runs(cls, N, H, W, which, work, offsets, total, counts, cum, e, null)

    for fn, tag in ((count, b"gpg_count_runs"), (write, b"gpg_write_runs")):
        for kw in (dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=2048, W=2049)):
            assert fn(**kw) == -1 and tag in err() and b"bad sizes" in err(), kw
        for which in (-1, 2):
            assert fn(which=which) == -1 and b"which" in err()
        assert fn(work=ctypes.c_void_p(12)) == -1 and b"aligned" in err()
        assert fn(N=0, cls=null, work=null) == 0
    assert write(total=-1) == -1 and b"bad sizes" in err()
    for name in ("cls", "runs", "work"):
        assert count(**{name: null}) == -1 and b"null" in err(), name
    for name in ("cls", "work", "offsets", "counts", "cum", "e"):
        assert write(**{name: null}) == -1 and b"null" in err(), name


def test_gtinfo_argument_validation_of_the_python_layer_needs_no_gpu():
    N, h, w = 2, 8, 8
    i32 = torch.int32
    a = dict(vis=torch.zeros(N, 3 * h, 3 * w, dtype=torch.int64), origin=(w, h), depth=torch.zeros(1, h, w), frame=torch.zeros(N, dtype=i32),
             ray=torch.ones(1, h, w, dtype=torch.float64), ray_index=torch.zeros(N, dtype=i32), delta=15.0)
    for what, bad in (("vis", a["vis"].int()), ("depth", a["depth"][:, :4]), ("depth", a["depth"].double()), ("frame", a["frame"].long()),
                      ("frame", a["frame"][:1]), ("ray", a["ray"].float()), ("ray_index", a["ray_index"][:1]), ("ray_index", a["ray_index"].long())):
        with pytest.raises(ValueError, match=what):
            gtinfo.classify(**dict(a, **{what: bad}))
    for origin in ((-1, 0), (0, -1), (2 * w + 1, 0), (0, 2 * h + 1)):
        with pytest.raises(ValueError, match="leaves the"):
            gtinfo.classify(**dict(a, origin=origin))
    with pytest.raises(ValueError, match="NaN"):
        gtinfo.classify(**dict(a, delta=float("nan")))
    with pytest.raises(ValueError, match="2\\^22"):
        gtinfo.classify(**dict(a, vis=torch.empty(N, 2048, 2049, dtype=torch.int64), ray=torch.empty(1, 2048, 2049, dtype=torch.float64), depth=None, origin=(0, 0)))
    for kw in ({}, dict(depth=None, frame=None)):
        with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
            gtinfo.classify(**dict(a, **kw))
    cls = torch.zeros(N, w, h, dtype=torch.uint8)
    for bad in (2, -1, None):
        with pytest.raises(ValueError, match="which"):
            gtinfo.encode_runs(cls, bad)
    with pytest.raises(ValueError, match="cls"):
        gtinfo.encode_runs(cls.int(), 0)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        gtinfo.encode_runs(cls, 0)
    models = cases.models()
    cameras = {(1, 1): dict(cam_K=cases.K, depth=np.zeros((480, 640), np.float32))}
    for kw, match in ((dict(margin=-0.5), "margin"), (dict(margin=float("inf")), "margin"), (dict(delta=float("nan")), "delta")):
        with pytest.raises(ValueError, match=match):
            gtinfo.GroundTruthInfo(models, cameras, **kw)
    with pytest.raises(ValueError, match="no cameras"):
        gtinfo.GroundTruthInfo(models, {})
    with pytest.raises(ValueError, match="frame size is unknown"):
        gtinfo.GroundTruthInfo(models, {(1, 1): dict(cam_K=cases.K)})
    with pytest.raises(ValueError, match="for every frame or for none"):
        gtinfo.GroundTruthInfo(models, {**cameras, (1, 2): dict(cam_K=cases.K, size=(480, 640))})
    # a canvas beyond the limits names the largest margin allowed, and that margin passes while the next thousandth does not
    with pytest.raises(ValueError, match="largest margin allowed for 480 x 640 frames is 41.3") as e:
        gtinfo.GroundTruthInfo(models, cameras, margin=50.0)
    largest = float(str(e.value).rsplit(" ", 1)[1])
    assert largest == gtinfo.largest_margin(480, 640)
    g = gtinfo.GroundTruthInfo(models, cameras, margin=largest, device="cpu")
    assert g.Hc * g.Wc < 2 ** 31 and (g.Hc, g.Wc, g.ox, g.oy) == gtinfo.canvas(480, 640, largest)
    with pytest.raises(ValueError, match="largest margin"):
        gtinfo.GroundTruthInfo(models, cameras, margin=largest + 0.001)
    assert gtinfo.canvas(96, 128, 1.0) == (288, 384, 128, 96) == gtinfo_ref.canvas(96, 128, 1.0) and gtinfo.canvas(96, 128, 0) == (96, 128, 0, 0)
    assert gtinfo.canvas(37, 23, 0.5) == (37 + 2 * 19, 23 + 2 * 12, 12, 19)                                       # rounded up to whole pixels
    rgb = gtinfo.GroundTruthInfo(models, {(1, 1): dict(cam_K=cases.K, size=(96, 128))}, device="cpu")           # no depth: the size is given
    assert (rgb.H, rgb.W, rgb.Hc, rgb.Wc) == (96, 128, 288, 384)
    gts = {(1, 1): [cases.ground_truth(cases.FRONT)]}
    with pytest.raises(ValueError, match="no camera"):
        rgb.compute({(1, 2): gts[(1, 1)]})
    with pytest.raises(ValueError, match="no model"):
        rgb.compute({(1, 1): [cases.ground_truth(cases.FRONT, obj_id=9)]})
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        rgb.compute(gts)
    assert gtinfo.box_xywh((3, 4, 3, 4)) == [3, 4, 1, 1] and gtinfo.box_xywh((-9, 2, 13, 5)) == [-9, 2, 23, 4]
    assert gtinfo.box_xywh((2 ** 30, 2 ** 30, -2 ** 30, -2 ** 30)) == [-1, -1, -1, -1]
