"""GPU: depth refinement (libgigapose_refine.so, gigapose_amd/refine.py).

gpf_face_normals, gpf_accumulate and gpf_update against the numpy restatement (gigapose_testing/refine_ref.py, written from the
header and held to rational arithmetic and to what a refiner is for by tests/test_refine_host.py) bit for bit -- sums, status
words, poses and their f32 copies: on keys from render.raster under every kind of box, on planted keys for every rule of the
association, at box areas around the workgroup's chunk, at the limits (65535 pairs in one call; a key buffer past 2^31 elements);
the invariances an integer sum must have; then DepthRefiner.refine end to end against the restatement's loop, and PoseScorer on
what it returns."""
import functools

import numpy as np
import pytest
import torch

from gigapose_testing import dist_ref, raster_ref, refine_ref
from gigapose_testing import refine_cases as cases

from gigapose_testing.gpu_cases import assert_bits, five_pairs
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = cases.H, cases.W


def device_accumulate(vis, c, poses, K, depth, frame, box, gate, scale):
    from gigapose_amd import refine

    sums, status = refine.accumulate(_t(np.asarray(vis)), _t(np.asarray(c, np.float64)), _t(np.asarray(poses, np.float64)),
                                     _t(np.asarray(K, np.float64)), _t(np.asarray(depth, np.float32)), _t(np.asarray(frame, np.int32)),
                                     _t(np.asarray(box, np.int32)), _t(np.asarray(gate, np.float64)), _t(np.asarray(scale, np.float64)))
    return sums.cpu().numpy(), status.cpu().numpy()


def check_accumulate(what, vis, c, poses, K, depth, frame, box, gate, scale):
    got = device_accumulate(vis, c, poses, K, depth, frame, box, gate, scale)
    want = refine_ref.accumulate(vis, c, poses, K, depth, frame, box, gate, scale)
    assert_bits(got[0], want[0], f"{what}: sums")
    assert_bits(got[1], want[1], f"{what}: status")
    return want


# ---------------------------------------------------------------------------------------------- 1. gpf_face_normals
def test_face_normals():
    from gigapose_amd import refine

    for name in ("boxes", "sphere"):
        v, f = cases.mesh(name)
        assert_bits(refine.face_normals(_t(v), _t(f)), refine_ref.face_normals(v, f), name)
    v, f = cases.mesh("boxes")
    bad = f.copy()
    bad[3, 1], bad[7, 0], bad[11, 2] = len(v), -1, 2 ** 31 - 1
    got = refine.face_normals(_t(v), _t(bad)).cpu().numpy()
    assert_bits(got, refine_ref.face_normals(v, bad), "an index out of range")
    assert np.isnan(got[[3, 7, 11]]).all() and np.isfinite(np.delete(got, [3, 7, 11], axis=0)).all()
    assert refine.face_normals(_t(v), _t(f[:0])).shape == (0, 3)


# ---------------------------------------------------------------------------------------------- 2. keys from render.raster
@functools.lru_cache(maxsize=None)
def rendered():
    """Five pairs on two frames: the three starts about GT on frame 0, two about GT2 on frame 1; keys from render.raster."""
    v, f = cases.mesh("boxes")
    poses, vis = five_pairs()
    depth = np.stack([cases.sensor_depth("boxes", 0), cases.sensor_depth("boxes", 1)])
    n = len(poses)
    return dict(vis=vis, c=refine_ref.face_normals(v, f), poses=poses, K=np.tile(cases.K, (n, 1)), depth=depth, frame=np.asarray([0, 0, 0, 1, 1], np.int32),
                gate=np.full(n, cases.GATE), scale=np.full(n, cases.SCALE))


def tight_boxes(vis):
    out = []
    for key in vis:
        ys, xs = np.nonzero(key != raster_ref.EMPTY_KEY)
        out.append((xs.min(), ys.min(), xs.max(), ys.max()))
    return np.asarray(out, np.int32)


def test_accumulate_on_rendered_keys_under_every_kind_of_box():
    r = rendered()
    n = len(r["poses"])
    whole = check_accumulate("whole frame", box=cases.whole_frame(n), **r)
    assert not whole[1].any() and (whole[0][:, refine_ref.COUNT] > 100).all() and (whole[0][:, 30:] == 0).all()
    tight = tight_boxes(r["vis"])
    assert_bits(check_accumulate("tight", box=tight, **r)[0], whole[0], "tight box = whole frame")
    cx, cy = (tight[:, 0] + tight[:, 2]) // 2, (tight[:, 1] + tight[:, 3]) // 2
    one = check_accumulate("1 x 1", box=np.stack([cx, cy, cx, cy], axis=1), **r)
    assert (one[0][:, refine_ref.COVERED] <= 1).all() and one[0][:, refine_ref.COVERED].any()
    for width in (63, 64, 65):
        check_accumulate(f"width {width}", box=np.stack([cx - 31, cy - 20, cx - 31 + width - 1, cy + 20], axis=1), **r)
    part = check_accumulate("partly outside", box=np.stack([cx, cy, cx + 500, cy + 500], axis=1), **r)
    assert part[0][:, refine_ref.COVERED].all()
    check_accumulate("negative corner", box=np.stack([cx - 500, cy - 500, cx, cy], axis=1), **r)
    for what, box in (("wholly outside, right", (W, 0, W + 50, H - 1)), ("wholly outside, above", (0, -40, W - 1, -1)), ("empty", (10, 10, 9, 20)),
                      ("inverted", (100, 80, 20, 10)), ("extreme", (-2 ** 31, -2 ** 31, -1, 2 ** 31 - 1))):
        got = check_accumulate(what, box=np.tile(np.asarray(box, np.int64).astype(np.int32), (n, 1)), **r)
        assert not got[0].any() and not got[1].any(), what
    mixed = tight.copy()
    mixed[1], mixed[3] = (5, 5, 4, 4), (0, 0, W - 1, H - 1)
    check_accumulate("a box of its own per pair", box=mixed, **r)


def test_accumulate_invariances():
    r = rendered()
    n = len(r["poses"])
    box = tight_boxes(r["vis"])
    whole = device_accumulate(box=box, **r)
    order = np.asarray([3, 0, 4, 2, 1])
    per_pair = {k: (v[order] if k != "depth" and k != "c" else v) for k, v in r.items()}
    got = device_accumulate(box=box[order], **per_pair)
    assert_bits(got[0], whole[0][order], "pairs permuted: sums")
    for a, b in ((0, 2), (2, 5)):
        part = device_accumulate(box=box[a:b], **{k: (v[a:b] if k != "depth" and k != "c" else v) for k, v in r.items()})
        assert_bits(part[0], whole[0][a:b], f"pairs {a}:{b} in a call of their own")
    again = device_accumulate(box=box, **r)
    assert_bits(again[0], whole[0], "a second run")


# ---------------------------------------------------------------------------------------------- 3. planted keys
def planted(n, h, w, seed, k=None, c=None, gate=30.0, scale=120.0, fill=1.0):
    """Random keys on an h x w frame for n pairs: faces of the three boxes, drawn depths 380 .. 420, measured depths within
    +-40 of them (so the gate of 30 cuts some), a share 1 - fill of the pixels uncovered."""
    rs = np.random.RandomState(seed)
    v, f = cases.mesh("boxes")
    c = refine_ref.face_normals(v, f) if c is None else c
    zr = rs.uniform(380, 420, (n, h, w)).astype(np.float32)
    face = rs.randint(0, len(c), (n, h, w)).astype(np.uint64)
    vis = (zr.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face
    vis[rs.uniform(size=vis.shape) > fill] = raster_ref.EMPTY_KEY
    depth = (zr[:1] + rs.uniform(-40, 40, (1, h, w))).astype(np.float32)
    poses = np.stack([cases.moved(cases.GT, rs.standard_normal(3), rs.uniform(0, 30), rs.uniform(-10, 10, 3)) for _ in range(n)])
    k = np.asarray([8000.0, 0.25, w / 2.0, 0.0, 7900.0, h / 2.0, 0.0, 0.0, 1.0]) if k is None else k
    return dict(vis=vis, c=c, poses=poses, K=np.tile(k, (n, 1)), depth=depth, frame=np.zeros(n, np.int32), gate=np.full(n, gate), scale=np.full(n, scale))


def test_accumulate_at_box_areas_around_the_workgroup_chunk():
    from gigapose_amd import refine

    C = refine.pixels_per_workgroup()
    w = 2 * C + 1                                                # a strip of one row: any area is a box (8193 pixels, fewer than 96 x 128)
    assert w <= H * W
    p = planted(4, 1, w, 11, fill=0.9)
    boxes = np.asarray([(0, 0, C - 2, 0), (0, 0, C - 1, 0), (0, 0, C, 0), (0, 0, 2 * C, 0)], np.int32)
    want = check_accumulate("areas C-1, C, C+1, 2C+1", box=boxes, **p)
    assert (want[0][:, refine_ref.COVERED] > 0.8 * np.asarray([C - 1, C, C + 1, 2 * C + 1])).all() and (want[0][:, refine_ref.COUNT] > C // 4).all()
    shifted = boxes + np.asarray([C - 1, 0, 0, 0], np.int32)     # ... and boxes that begin in the middle of a chunk of the frame
    check_accumulate("boxes from x = C-1", box=shifted, **p)
    p2 = planted(3, 3, C // 2 + 5, 12)                           # rows shorter than a chunk: a chunk spans rows
    check_accumulate("three rows", box=np.asarray([(0, 0, C // 2 + 4, 2), (1, 0, C // 2 + 3, 2), (7, 1, C // 2, 2)], np.int32), **p2)


def test_accumulate_on_planted_keys_every_rule_with_its_status_bit():
    v, f = cases.mesh("boxes")
    c = refine_ref.face_normals(v, f)
    c = np.concatenate([c, [[0.0, 0.0, 0.0], [np.nan, 1.0, 1.0], [np.inf, 0.0, 0.0]]])
    F = len(c)
    n, h, w = 9, 8, 16
    p = planted(n, h, w, 21, k=np.asarray([114.0, 0.0, 8.0, 0.0, 115.0, 4.0, 0.0, 0.0, 1.0]), c=c, gate=30.0)
    zero, nan, inf = F - 3, F - 2, F - 1
    p["vis"] &= ~np.uint64(0xFFFFFFFF)
    p["vis"] |= np.random.RandomState(3).randint(0, F - 3, p["vis"].shape).astype(np.uint64)
    p["depth"] = np.tile(p["depth"], (2, 1, 1))                  # two frames; frame 1 holds the special measurements
    p["poses"][:] = cases.GT
    p["poses"][:, :3, 3] = (0.0, 0.0, 400.0)

    def key(z, face):
        return (np.uint64(np.asarray([z], np.float32).view(np.uint32)[0]) << np.uint64(32)) | np.uint64(face)

    vis, d1 = p["vis"], p["depth"][1]
    vis[1, 2, 3] = raster_ref.EMPTY_KEY                          # pair 1: uncovered pixels
    vis[1, 5, :4] = raster_ref.EMPTY_KEY
    vis[2, 1, 1], vis[2, 7, 15] = key(400.0, F), key(400.0, 0xFFFFFFFE)      # pair 2: f >= F
    p["frame"][3] = 1                                            # pair 3: dm = 0, negative, NaN, inf
    d1[:] = p["depth"][0]
    d1[0, 0], d1[0, 1], d1[0, 2], d1[0, 3], d1[0, 4] = 0.0, -400.0, np.nan, np.inf, -np.inf
    p["frame"][4] = 1                                            # pair 4: |dm - zr| exactly at the gate and one f32 above it
    vis[4, 3, 5], vis[4, 3, 6], vis[4, 3, 7], vis[4, 3, 8] = key(400.0, 1), key(400.0, 1), key(400.0, 1), key(400.0, 1)
    d1[3, 5], d1[3, 6] = 430.0, np.nextafter(np.float32(430.0), np.float32(500))
    d1[3, 7], d1[3, 8] = 370.0, np.nextafter(np.float32(370.0), np.float32(0))
    vis[5, 4, 4] = key(3000.0, 2)                                # pair 5: y.y beyond 16 (a drawn point 2600 units behind the object)
    p["depth"][0][4, 4] = 3010.0
    vis[6, 6, 6] = key(400.0, zero)                              # pair 6: a zero normal -- not associated, no bit
    vis[7, 2, 2], vis[7, 2, 3] = key(400.0, nan), key(400.0, inf)            # pair 7: a normal that is not finite
    p["frame"][8] = 2                                            # pair 8: a frame index outside the depth stack
    want = check_accumulate("planted", box=cases.whole_frame(n, h, w), **p)
    R, B = refine_ref.RANGE, refine_ref.BAD_INDEX
    assert want[1].tolist() == [0, 0, B, 0, 0, R, 0, B, B]
    px = h * w
    assert want[0][:, refine_ref.COVERED].tolist() == [px, px - 5, px, px, px, px, px, px, 0]
    base = lambda pair, frame: refine_ref.accumulate(p["vis"][pair:pair + 1], c, p["poses"][:1], p["K"][:1], p["depth"], [frame], cases.whole_frame(1, h, w),
                                                     [30.0], [120.0])[0][0]
    # the gate: of the four planted pixels the two AT the gate count, the two one f32 beyond it do not
    at = [refine_ref.pixel_terms(vis[4, 3, x:x + 1], d1[3, x:x + 1], [x], [3], c, p["poses"][4], p["K"][4], 30.0, 120.0)[0][0, refine_ref.COUNT] for x in (5, 6, 7, 8)]
    assert at == [1, 0, 1, 0]
    assert int(want[0][8].any()) == 0 and (base(3, 1) == want[0][3]).all()
    for pair in range(8):
        assert 0 < want[0][pair, refine_ref.COUNT] < want[0][pair, refine_ref.COVERED], pair


# ---------------------------------------------------------------------------------------------- 4. limits
def test_accumulate_65535_pairs_in_one_call():
    n, reps = 5, 13107
    assert n * reps == 65535
    p = planted(n, 8, 8, 31, k=np.asarray([114.0, 0.0, 4.0, 0.0, 115.0, 4.0, 0.0, 0.0, 1.0]), fill=0.8)
    p["poses"][:, :3, 3] = (0.0, 0.0, 400.0)
    box = np.asarray([(0, 0, 7, 7), (1, 1, 6, 6), (0, 0, 7, 3), (-3, 2, 20, 20), (4, 4, 4, 4)], np.int32)
    want = refine_ref.accumulate(box=box, **p)
    assert want[0][:4, refine_ref.COUNT].all()
    tiled = {k: (np.tile(v, (reps,) + (1,) * (v.ndim - 1)) if k not in ("depth", "c") else v) for k, v in p.items()}
    got = device_accumulate(box=np.tile(box, (reps, 1)), **tiled)
    assert_bits(got[0], np.tile(want[0], (reps, 1)), "65535 pairs: sums")
    assert_bits(got[1], np.tile(want[1], reps), "65535 pairs: status")


def test_accumulate_addresses_a_key_buffer_past_2_to_the_31_elements():
    """513 pairs of 2048 x 2048: the LAST pair's keys begin 2^31 elements (16 GiB) into the buffer; only its box is non-empty, so
    only its plane is ever read and only its plane is initialised."""
    from gigapose_amd import refine

    n, side = 513, 2048
    assert (n - 1) * side * side >= 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    assert free > n * side * side * 8 + (1 << 30), "the device has too little free memory for this case"
    p = planted(1, 48, 48, 41, k=np.asarray([8000.0, 0.0, 2020.0, 0.0, 8000.0, 2020.0, 0.0, 0.0, 1.0]), fill=0.9)
    plane = np.full((side, side), raster_ref.EMPTY_KEY, np.uint64)
    plane[2000:2048, 2000:2048] = p["vis"][0]
    depth = np.zeros((1, side, side), np.float32)
    depth[0, 2000:2048, 2000:2048] = p["depth"][0]
    box1 = np.asarray([[1990, 1995, 5000, 2047]], np.int32)
    want = refine_ref.accumulate(plane[None], p["c"], p["poses"], p["K"], depth, [0], box1, p["gate"], p["scale"])
    assert want[0][0, refine_ref.COUNT] > 1000
    vis = torch.empty(n, side, side, dtype=torch.int64, device=DEV)
    vis[-1].copy_(_t(plane))
    box = np.tile(np.asarray([0, 0, -1, -1], np.int32), (n, 1))
    box[-1] = box1[0]
    rep = lambda a: _t(np.tile(a, (n,) + (1,) * (a.ndim - 1)))
    sums, status = refine.accumulate(vis, _t(p["c"]), rep(p["poses"]), rep(p["K"]), _t(depth), _t(np.zeros(n, np.int32)), _t(box), rep(p["gate"]),
                                     rep(p["scale"]))
    sums, status = sums.cpu().numpy(), status.cpu().numpy()
    del vis
    torch.cuda.empty_cache()
    assert not sums[:-1].any() and not status[:-1].any()
    assert_bits(sums[-1:], want[0], "the last pair: sums")
    assert_bits(status[-1:], want[1], "the last pair: status")


# ---------------------------------------------------------------------------------------------- 5. gpf_update
def device_update(sums, clipped, scale, start, poses, poses32, state, **step):
    from gigapose_amd import refine

    P, P32, S = _t(np.asarray(poses, np.float64)), _t(np.asarray(poses32, np.float32)), _t(np.asarray(state, np.int32))
    refine.update(_t(np.asarray(sums, np.int64)), None if clipped is None else _t(np.asarray(clipped, np.int32)), _t(np.asarray(scale, np.float64)),
                  None if start is None else _t(np.asarray(start, np.float64)), P, P32, S, **step)
    return P.cpu().numpy(), P32.cpu().numpy(), S.cpu().numpy()


def test_update_on_accumulated_and_planted_sums():
    r = rendered()
    n = len(r["poses"])
    sums, _ = refine_ref.accumulate(box=cases.whole_frame(n), **r)
    step = dict(min_points=32, min_pivot=1e-3, damping=0.0, tol2=1e-12)
    for damping in (0.0, 1e-3):
        step["damping"] = damping
        got = device_update(sums, np.zeros(n, np.int32), r["scale"], r["poses"], r["poses"], r["poses"].astype(np.float32), np.zeros(n, np.int32), **step)
        want = refine_ref.update(sums, np.zeros(n, np.int32), r["scale"], r["poses"], poses=r["poses"], state=np.zeros(n, np.int32), **step)
        for g, w_, what in zip(got, want, ("poses", "f32 copy", "state")):
            assert_bits(g, w_, f"accumulated sums, damping {damping}: {what}")
        assert not want[2].any() and (want[0] != r["poses"]).any()
    psums, bits, state, clipped = cases.planted_sums()
    m = len(psums)
    rs = np.random.RandomState(9)
    start = np.stack([cases.rigid(cases.rot(rs.standard_normal(3), 30 * i), rs.uniform(-50, 50, 3)) for i in range(m)])
    poses = np.stack([cases.rigid(cases.rot(rs.standard_normal(3), 20 + i), rs.uniform(-50, 50, 3)) for i in range(m)])
    p32 = poses.astype(np.float32)
    p32[9] = 7.0                                                 # a stopped pair: even a stale f32 copy stays
    step = dict(min_points=32, min_pivot=1e-3, damping=0.0, tol2=1e-4)
    for with_start in (True, False):
        got = device_update(psums, clipped, np.full(m, 100.0), start if with_start else None, poses, p32, state, **step)
        want = refine_ref.update(psums, clipped, np.full(m, 100.0), start if with_start else None, poses=poses, state=state, **step)
        assert_bits(got[0], want[0], f"planted sums, start {with_start}: poses")
        assert_bits(got[2], want[2], f"planted sums, start {with_start}: state")
        assert got[2].tolist() == bits.tolist()
        assert (got[1][9] == 7.0).all() and (got[0][9] == poses[9]).all()
        moved = [0, 1] + ([2, 3, 4, 5, 6, 7, 8, 10] if with_start else [])
        assert_bits(got[1][moved], want[0][moved].astype(np.float32), "the f32 copy of every pose that was written")
        if not with_start:
            assert_bits(got[1][[2, 3, 4, 5, 6, 7, 8, 10]], p32[[2, 3, 4, 5, 6, 7, 8, 10]], "a pair that stops without a start pose keeps its copy")
    got = device_update(psums, None, np.full(m, 100.0), start, poses, p32, state, **step)          # no clipped counts: pair 10 moves
    assert got[2][10] == 0 and (got[0][10] != poses[10]).any() and got[2][:10].tolist() == bits[:10].tolist()


# ---------------------------------------------------------------------------------------------- 6. DepthRefiner end to end
K2 = np.asarray([120.0, 0.0, 60.5, 0.0, 119.0, 50.25, 0.0, 0.0, 1.0])


def estimates_of(poses, scene, im, obj):
    return [dict(scene_id=scene, im_id=im, obj_id=obj, score=0.9 - 0.01 * i, R=p[:3, :3].copy(), t=p[:3, 3].copy()) for i, p in enumerate(poses)]


@functools.lru_cache(maxsize=None)
def scene():
    boxes, sphere = cases.mesh("boxes"), cases.mesh("sphere")
    models = {1: dict(vertices=boxes[0], faces=boxes[1], diameter=cases.SCALE), 2: dict(vertices=sphere[0], faces=sphere[1], diameter=cases.SCALE)}
    depth2 = cases.depth_of(cases.draw(*boxes, cases.GT2, K2))
    cameras = {(1, 1): dict(cam_K=cases.K, depth=cases.sensor_depth("boxes")), (1, 2): dict(cam_K=K2, depth=depth2),
               (1, 3): dict(cam_K=cases.K, depth=cases.sensor_depth("sphere"))}
    second = np.stack([cases.moved(cases.GT2, [1, 1, 0], 5, (3, 2, -6)), cases.moved(cases.GT2, [0, 1, 2], 10, (-4, 5, 9))])
    est = (estimates_of(cases.starts(), 1, 1, 1) + estimates_of(second, 1, 2, 1) + estimates_of(cases.starts(), 1, 3, 2)
           + estimates_of(cases.wrong_starts(), 1, 1, 1))
    n = len(second)
    ref2 = refine_ref.refine(*boxes, second, np.tile(K2, (n, 1)), depth2[None], np.zeros(n, np.int32), cases.whole_frame(n), np.full(n, cases.GATE),
                             np.full(n, cases.SCALE), cases.ITERS, 32, 1e-3, 0.0, cases.STEP["tol2"], H, W)
    refs = [cases.run("boxes", "right"), ref2, cases.run("sphere", "right"), cases.run("boxes", "wrong")]
    return models, cameras, est, refs, second


def check_refined(out, est, refs, what):
    from gigapose_amd import refine

    i = 0
    for ref in refs:
        rms = refine.rms_from_sums(ref["sums"], np.full(len(ref["poses"]), cases.SCALE))
        for j, pose in enumerate(ref["poses"]):
            o = out[i]
            assert_bits(o["R"], pose[:3, :3].copy(), f"{what}: estimate {i}: R")
            assert_bits(o["t"], pose[:3, 3].copy(), f"{what}: estimate {i}: t")
            assert o["status"] == int(ref["state"][j]) | int(ref["status"][j]), (what, i, o["status"])
            assert (o["inliers"], o["covered"]) == (int(ref["sums"][j, refine_ref.COUNT]), int(ref["sums"][j, refine_ref.COVERED])), (what, i)
            assert np.float64(o["rms"]).tobytes() == rms[j].tobytes(), (what, i)
            assert all(o[k] == est[i][k] for k in ("scene_id", "im_id", "obj_id", "score"))
            i += 1
    assert i == len(out)


def test_depth_refiner_equals_the_restatement_loop():
    from gigapose_amd import refine

    models, cameras, est, refs, second = scene()
    refiner = refine.DepthRefiner(models, cameras, iters=cases.ITERS, gate=0.25, min_points=32, min_pivot=1e-3, damping=0.0, tol=1e-6, box="frame")
    out = refiner.refine(est)
    check_refined(out, est, refs, "one chunk")
    v = models[1]["vertices"]
    for i, s in enumerate(cases.starts()):                       # what the host test asks of the restatement, of the device
        assert cases.deviation(v, cases.rigid(out[i]["R"], out[i]["t"])) < 0.01 * cases.deviation(v, s)
    for i in (5, 6, 7):                                          # the sphere: degenerate, the INPUT pose comes back
        assert out[i]["status"] & refine.STOP == refine.DEGENERATE
        assert_bits(out[i]["R"], est[i]["R"], "the input R")
        assert_bits(out[i]["t"], est[i]["t"], "the input t")
    right, wrong = out[:3], out[8:]
    assert max(o["inliers"] / o["covered"] for o in wrong) < min(o["inliers"] / o["covered"] for o in right)
    assert min(o["rms"] for o in wrong) > max(o["rms"] for o in right)
    chunked = refine.DepthRefiner(models, cameras, iters=cases.ITERS, gate=0.25, min_points=32, min_pivot=1e-3, damping=0.0, tol=1e-6, box="frame",
                                  pairs_per_call=2).refine(est)
    check_refined(chunked, est, refs, "chunks of 2")
    loose = refine.DepthRefiner(models, cameras, iters=cases.ITERS, gate=0.25, min_points=32, min_pivot=1e-5, tol=1e-6, box="frame").refine(est[5:8])
    check_refined(loose, est[5:8], [cases.run("sphere", "right", min_pivot=1e-5)], "the sphere at min_pivot 1e-5")
    # the projected box (the default) and the caller's boxes hold every pixel the model draws: the same poses as the whole frame
    boxed = refine.DepthRefiner(models, cameras, iters=cases.ITERS, min_pivot=1e-3, tol=1e-6, margin=24).refine(est[:5])
    given = refine.DepthRefiner(models, cameras, iters=cases.ITERS, min_pivot=1e-3, tol=1e-6).refine(est[:5], boxes=np.tile(np.asarray([20, 5, 120, 95]), (5, 1)))
    for a, b, c_ in zip(out[:5], boxed, given):
        for o in (b, c_):
            assert_bits(o["R"], a["R"], "a box that holds the model: R")
            assert_bits(o["t"], a["t"], "a box that holds the model: t")
            assert (o["inliers"], o["status"]) == (a["inliers"], a["status"])


def test_refined_estimates_score_above_the_coarse_ones(tmp_path):
    """Three boxes at two ground-truth poses, the depth of each image from MeshRenderer with a wall behind, rounded to integers as a
    depth PNG holds them; csv -> refine -> csv -> PoseScorer.score_csv."""
    from gigapose_amd import evaluate, refine, render

    v, f = cases.mesh("boxes")
    diameter = dist_ref.diameter(v)
    gts_p = [cases.GT, cases.GT2]
    r = render.MeshRenderer(H, W, cases.K)(_t(v), _t(f), None, _t(np.stack(gts_p).astype(np.float32)), colour=(255, 255, 255))
    depth = r["depth"].cpu().numpy()
    depth = np.rint(np.where(depth > 0, depth, np.float32(cases.WALL))).astype(np.float32)
    models = {1: dict(vertices=v, faces=f, diameter=diameter)}
    cameras = {(1, i): dict(cam_K=cases.K, depth=depth[i]) for i in range(2)}
    targets = [dict(scene_id=1, im_id=i, obj_id=1, inst_count=1) for i in range(2)]
    gts = {(1, i): [dict(obj_id=1, cam_R_m2c=g[:3, :3].reshape(-1), cam_t_m2c=g[:3, 3])] for i, g in enumerate(gts_p)}
    coarse = (estimates_of([cases.moved(cases.GT, [2, -1, 1], 8, (5, 4, -12))], 1, 0, 1)
              + estimates_of([cases.moved(cases.GT2, [0, 1, 2], 10, (-4, 5, 9))], 1, 1, 1))
    path = refine.write_estimates(tmp_path / "coarse.csv", coarse)
    refined = refine.DepthRefiner(models, cameras, iters=cases.ITERS).refine(evaluate.read_estimates(path))
    assert all(not e["status"] & refine.STOP and e["inliers"] == e["covered"] > 200 for e in refined)
    out = refine.write_estimates(tmp_path / "refined.csv", refined)
    scorer = evaluate.PoseScorer(models, targets, gts, cameras)
    before, after = scorer.score_csv(path), scorer.score_csv(out)
    errs = scorer.errors(evaluate.read_estimates(out))
    print("coarse", {k: before[k] for k in ("ar_mssd", "ar_mspd", "ar_vsd", "ar")}, "refined", {k: after[k] for k in ("ar_mssd", "ar_mspd", "ar_vsd", "ar")},
          "mssd", [float(e["mssd"][0, 0]) for _, e in errs], "mspd", [float(e["mspd"][0, 0]) for _, e in errs])
    assert after["ar_mssd"] == 1.0 and after["ar_mspd"] == 1.0
    assert after["ar_mssd"] + after["ar_mspd"] > before["ar_mssd"] + before["ar_mspd"]
    assert after["ar_mssd"] > before["ar_mssd"] and after["ar_mspd"] >= before["ar_mspd"]
