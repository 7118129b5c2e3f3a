"""Inputs for the tests of the ground-truth visibility stage (gigapose_amd/gtinfo.py, gigapose_testing/gtinfo_ref.py), shared by the
CPU and the GPU suite: planted keys, depths and rays for every branch of the visibility rule (every comparison on them is exact),
object pixels planted inside the frame, outside it and on the edges of frame and canvas, masks for the run lists, and the scene of
refine_cases (the three-box object, 96 x 128) with several ground truths that hide each other or leave the frame."""
import functools

import numpy as np

from . import gtinfo_ref, raster_ref
from . import maskfit_cases as mc
from . import refine_cases as rc
from .verify_cases import key_of

DELTA = 10.0                                         # of the planted cases: dyadic
TINY = np.float32(2.0 ** -60)                        # a measurement > 0 whose ray distance vanishes against 10 in float64
OFF_AXIS = 1.25                                      # the ray length at a = 0.75, b = 0: sqrt(0.75^2 + 1)
NAN_KEY = (np.uint64(0x7FC00000) << np.uint64(32)) | np.uint64(5)       # dm is a NaN, the key is not all ones
FRAMES = ((1, 1), (1, 9), (7, 1), (37, 23), (65, 63))


def planted_pixels():
    """(name, key, sensor depth, ray, object, visible, valid) at DELTA."""
    f32, nxt = np.float32, float(np.nextafter(OFF_AXIS, 2.0))
    return [("not covered", raster_ref.EMPTY_KEY, f32(300), 1.0, 0, 0, 0),
            ("dm = 0", key_of(0.0, 1), f32(300), 1.0, 0, 0, 0), ("dm < 0", key_of(-300.0, 2), f32(300), 1.0, 0, 0, 0),
            ("dm NaN", NAN_KEY, f32(300), 1.0, 0, 0, 0), ("dm +inf", key_of(np.inf, 3), f32(300), 1.0, 0, 0, 0),
            ("in front of the sensor's surface", key_of(200.0), f32(300), 1.0, 1, 1, 1), ("on it", key_of(300.0), f32(300), 1.0, 1, 1, 1),
            ("hidden", key_of(300.0), f32(200), 1.0, 1, 0, 1),
            ("dt = 0", key_of(300.0), f32(0), 1.0, 1, 1, 0), ("dt < 0", key_of(300.0), f32(-200), 1.0, 1, 1, 0),
            ("dt NaN", key_of(300.0), f32(np.nan), 1.0, 1, 1, 0), ("dt +inf", key_of(300.0), f32(np.inf), 1.0, 1, 1, 0),
            ("dt -inf", key_of(300.0), f32(-np.inf), 1.0, 1, 1, 0),
            # Dm = 8 * 1.25 = 10 and Dt = 2^-60 * 1.25: Dm - Dt rounds to 10 = delta exactly
            ("Dm - Dt exactly delta", key_of(8.0), TINY, OFF_AXIS, 1, 1, 1),
            # Dm = 8 * nextafter(1.25) = nextafter(10): one float64 step above delta
            ("one step above delta", key_of(8.0), TINY, nxt, 1, 0, 1),
            ("308 - 300 off the axis: 10", key_of(308.0), f32(300), OFF_AXIS, 1, 1, 1),
            # the z-depths differ by 9 <= delta, the ray distances by 11.25: the decisive pixel of z-depth in place of the ray distance
            ("309 - 300 off the axis: 11.25", key_of(309.0), f32(300), OFF_AXIS, 1, 0, 1)]


def origins(H, W):
    """The canvases a frame is tested on: the frame itself, one frame size per side (margin 1.0) and an odd one."""
    return (((H, W), (0, 0)), ((3 * H, 3 * W), (W, H)), ((H + 70, W + 5), (3, 66)))


def planted_case(H, W, canvas, origin, seed=0, with_depth=True):
    """One instance per planted pixel (its key at a pixel of the frame, its depth and ray at that pixel of a frame and a ray map of
    its own), then instances of plain object pixels over a mixed depth: only outside the frame, only inside, on the edges of the
    frame from both sides, on the corners and edges of the canvas, a dense half, nothing.  -> the arguments of classify as a dict,
    + "expect": per planted instance (object, visible, valid), + "names"."""
    (Hc, Wc), (ox, oy) = canvas, origin
    rs = np.random.RandomState(100 + seed)
    kinds = planted_pixels()
    P = len(kinds)
    depth, ray = np.zeros((P + 1, H, W), np.float32), np.ones((P + 1, H, W), np.float64)
    keys = []
    for i, (_, key, dt, r, _, _, _) in enumerate(kinds):
        x, y = rs.randint(W), rs.randint(H)
        k = np.full((Hc, Wc), raster_ref.EMPTY_KEY, np.uint64)
        k[y + oy, x + ox], depth[i, y, x], ray[i, y, x] = key, dt, r
        keys.append(k)
    depth[P] = rs.choice(np.asarray([0.0, 200.0, 300.0, 400.0, np.nan], np.float32), size=(H, W))
    ray[P] = 1.0 + rs.randint(0, 9, (H, W)) / 16.0
    inside = np.zeros((Hc, Wc), bool)
    inside[oy:oy + H, ox:ox + W] = True
    plain = key_of(300.0, 7)
    shapes = {"only outside": ~inside & (rs.uniform(size=(Hc, Wc)) < 0.3), "only inside": inside & (rs.uniform(size=(Hc, Wc)) < 0.5),
              "dense half": rs.uniform(size=(Hc, Wc)) < 0.5, "nothing": np.zeros((Hc, Wc), bool)}
    edges = np.zeros((Hc, Wc), bool)
    for x, y in ((0, H // 2), (W - 1, H // 2), (W // 2, 0), (W // 2, H - 1), (-1, H // 2), (W, H // 2), (W // 2, -1), (W // 2, H)):
        if 0 <= x + ox < Wc and 0 <= y + oy < Hc:
            edges[y + oy, x + ox] = True
    shapes["frame edges"] = edges
    rim = np.zeros((Hc, Wc), bool)
    rim[0, 0], rim[0, Wc - 1], rim[Hc - 1, 0], rim[Hc - 1, Wc - 1] = True, True, True, True
    rim[0, Wc // 2], rim[Hc - 1, Wc // 2], rim[Hc // 2, 0], rim[Hc // 2, Wc - 1] = True, True, True, True
    shapes["canvas edges"] = rim
    for m in shapes.values():
        keys.append(np.where(m, plain, raster_ref.EMPTY_KEY).astype(np.uint64))
    n_shapes = len(shapes)
    case = dict(vis=np.stack(keys), origin=(ox, oy), depth=depth if with_depth else None,
                frame=np.concatenate([np.arange(P), np.full(n_shapes, P)]).astype(np.int32), ray=ray,
                ray_index=np.concatenate([np.arange(P), np.full(n_shapes, P)]).astype(np.int32), delta=DELTA)
    for a in (case["vis"], depth, ray, case["frame"], case["ray_index"]):
        a.setflags(write=False)
    return dict(args=case, expect=[k[4:] for k in kinds], names=[k[0] for k in kinds] + list(shapes), H=H, W=W)


def call(case, **changes):
    """The positional arguments of gtinfo_ref.classify / gtinfo.classify."""
    a = dict(case["args"], **changes)
    return a["vis"], a["origin"], a["depth"], a["frame"], a["ray"], a["ray_index"], a["delta"]


# ------------------------------------------------------------------------------------------------ masks for the run lists
def run_masks():
    """(name, dense mask (h,w) bool): maskfit_cases.host_masks() and the lists' own edge cases."""
    out = list(mc.host_masks())
    h, w = 5, 7
    first, last = np.zeros((h, w), bool), np.zeros((h, w), bool)
    first[0, 0], last[h - 1, w - 1] = True, True
    yy, xx = np.mgrid[0:h, 0:w]
    three = np.zeros((h, w), bool)
    three[3:, 2], three[:, 3], three[:2, 4] = True, True, True
    out += [("all zeros", np.zeros((h, w), bool)), ("all ones", np.ones((h, w), bool)), ("pixel 0", first), ("the last pixel", last),
            ("checkerboard", (yy + xx) % 2 == 1), ("checkerboard from pixel 0", (yy + xx) % 2 == 0), ("one run across three columns", three)]
    return out


def cls_of(obj, visible=None):
    """Dense masks (N,H,W) bool -> cls (N,W,H) u8: bit 0 from obj, bit 1 from visible (default: obj)."""
    obj = np.asarray(obj, bool)
    visible = obj if visible is None else np.asarray(visible, bool)
    return np.ascontiguousarray((obj * gtinfo_ref.CLS_OBJECT + visible * gtinfo_ref.CLS_VISIBLE).astype(np.uint8).transpose(0, 2, 1))


def chunk_edge_bits(HW, C, rs):
    """Column-major bits of length HW with transitions planted at p = 0, C-1, C, C+1 and HW-1 (those that exist) among random runs."""
    v = np.repeat(rs.randint(0, 2, HW // 7 + 2), 7)[:HW].astype(bool)
    for p in sorted({0, C - 1, C, C + 1, HW - 1}):                  # ascending: v[p - 1] is final when v[p] is set against it
        if 0 <= p < HW:
            v[p] = not (v[p - 1] if p else False)
    return v


# ------------------------------------------------------------------------------------------------ the scene
H, W, K, SCALE = rc.H, rc.W, rc.K, rc.SCALE
Z = [0, 0, 1]
FREE = rc.moved(rc.GT, Z, 0, (-140.0, 60.0, 0.0))                # beside the others: nothing hides it
FRONT = rc.GT
BEHIND = rc.moved(rc.GT, Z, 0, (40.0, 0.0, 110.0))               # partly behind FRONT
HALF_OUT = rc.rigid(rc.GT[:3, :3], (-64.0 / K[0] * 400.0, 20.0, 400.0))     # its origin projects onto the frame's left edge
BURIED = rc.rigid(rc.GT[:3, :3], rc.GT[:3, 3] * 1.3)             # FRONT pushed back along its viewing ray: wholly behind it
SCENE = (("free", FREE), ("front", FRONT), ("behind", BEHIND))
POSES = dict(SCENE + (("half out", HALF_OUT), ("buried", BURIED)))
OCCLUDED_SCENE = ("free", "front", "behind", "buried")           # one ground truth is less than 10 % visible


def ground_truth(pose, obj_id=1):
    return dict(obj_id=obj_id, cam_R_m2c=np.asarray(pose)[:3, :3].reshape(9).tolist(), cam_t_m2c=np.asarray(pose)[:3, 3].tolist())


def models():
    v, f = rc.mesh("boxes")
    return {1: dict(vertices=v, faces=f, diameter=SCALE)}


@functools.lru_cache(maxsize=None)
def drawn(name, margin=1.0):
    """The keys of a named pose on the canvas of `margin` -> (Hc,Wc) u64, read-only."""
    pose = POSES[name]
    v, f = rc.mesh("boxes")
    vis, clipped, _ = gtinfo_ref.draw_on_canvas(v, f, pose[None], K, H, W, margin)
    assert not clipped.any()
    vis[0].setflags(write=False)
    return vis[0]


def window(canvas_array, margin=1.0):
    _, _, ox, oy = gtinfo_ref.canvas(H, W, margin)
    return canvas_array[oy:oy + H, ox:ox + W]


@functools.lru_cache(maxsize=None)
def z_buffer(names=tuple(n for n, _ in SCENE), margin=1.0):
    """The sensor's depth: the smallest drawn depth over the named instances in the frame window of their canvas drawings, 0 where
    nothing is drawn (no wall: what no instance covers is not measured)."""
    z = np.stack([np.where(window(drawn(n, margin), margin) != raster_ref.EMPTY_KEY, gtinfo_ref.key_depth(window(drawn(n, margin), margin)), np.inf)
                  for n in names]).min(axis=0)
    z = np.where(np.isfinite(z), z, 0).astype(np.float32)
    z.setflags(write=False)
    return z


def scene(depth=None, names=tuple(n for n, _ in SCENE)):
    """-> models, cameras, gts of one image (1, 1) with the named instances; depth: the sensor's (default: their z-buffer)."""
    d = z_buffer(names) if depth is None else depth
    return models(), {(1, 1): dict(cam_K=K, depth=d)}, {(1, 1): [ground_truth(POSES[n]) for n in names]}
