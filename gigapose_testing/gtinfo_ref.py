"""libgigapose_gtinfo.so restated in numpy from the description in include/gigapose_gtinfo.h (the definitions there are the
contract): the class of every pixel of a drawn ground truth against the sensor's depth, the four counts, the two boxes, and the
run-length lists of the two masks.  The GPU tests compare the kernels with this bit for bit; compute() at the end is
GroundTruthInfo.compute's host half over raster_ref's rasteriser, sharing nothing with gigapose_amd/gtinfo.py but the constants.

`variant` selects a deliberately WRONG version (tests/test_gtinfo_host.py shows that its checks reject each): None is the
contract."""
import numpy as np

from . import raster_ref

INFO, BOX = 4, 8
PX_ALL, PX_FRAME, PX_VALID, PX_VISIB = 0, 1, 2, 3
BOX_EMPTY = (2 ** 30, 2 ** 30, -2 ** 30, -2 ** 30)
CLS_OBJECT, CLS_VISIBLE = 1, 2
BAD_FRAME, BAD_RAY = 1, 2
CHUNK = 4096                                         # gpg_pixels_per_workgroup(): only the variant "chunk_start_zero" depends on it
VARIANTS = ("row_major", "strict_delta", "z_depth", "all_from_frame", "unmeasured_hidden", "first_run_ones", "last_missing",
            "chunk_start_zero")


def key_depth(vis):
    """The f32 whose bits are the high word of each key."""
    return (np.asarray(vis, np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def clean_depth(d):
    """A sensor depth that is negative, NaN or infinite counts as 0."""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((d > 0) & (d < np.inf), d, np.float32(0)).astype(np.float32)


def corners(mask, ox, oy):
    """min x, min y, max x, max y of the set pixels of a canvas-sized mask in frame coordinates; the initial values where empty."""
    ys, xs = np.nonzero(mask)
    return BOX_EMPTY if not len(xs) else (xs.min() - ox, ys.min() - oy, xs.max() - ox, ys.max() - oy)


def classify(vis, origin, depth, frame, ray, ray_index, delta, variant=None):
    """vis (N,Hc,Wc) u64, origin (ox, oy), depth (M,H,W) f32 or None, frame (N) (ignored without depth), ray (R,H,W) f64, ray_index
    (N), delta -> cls (N,W,H) u8, info (N,4) int64, box (N,8) int32, status (N) int32."""
    vis = np.asarray(vis).view(np.uint64)
    ray = np.asarray(ray, np.float64)
    N, (R, H, W), (ox, oy) = len(vis), ray.shape, (int(v) for v in origin)
    cls, info = np.zeros((N, W, H), np.uint8), np.zeros((N, INFO), np.int64)
    box, status = np.tile(np.asarray(BOX_EMPTY * 2, np.int32), (N, 1)), np.zeros(N, np.int32)
    for n in range(N):
        bad = 0
        if depth is not None and not 0 <= int(frame[n]) < len(depth):
            bad |= BAD_FRAME
        if not 0 <= int(ray_index[n]) < R:
            bad |= BAD_RAY
        if bad:
            status[n] = bad
            continue
        dm = key_depth(vis[n])
        with np.errstate(invalid="ignore"):
            obj = (vis[n] != raster_ref.EMPTY_KEY) & (dm > 0) & (dm < np.inf)
        window = np.zeros_like(obj)
        window[oy:oy + H, ox:ox + W] = obj[oy:oy + H, ox:ox + W]
        dt = np.zeros((H, W), np.float32) if depth is None else clean_depth(depth[int(frame[n])])
        r = np.ones((H, W)) if variant == "z_depth" else ray[int(ray_index[n])]
        with np.errstate(all="ignore"):
            Dm, Dt = dm[oy:oy + H, ox:ox + W].astype(np.float64) * r, dt.astype(np.float64) * r
            near = (Dm - Dt) < delta if variant == "strict_delta" else (Dm - Dt) <= delta
        inside = window[oy:oy + H, ox:ox + W]
        seen = inside & ((dt > 0) & near if variant == "unmeasured_hidden" else ((dt > 0) & near) | (dt == 0))
        visible = np.zeros_like(obj)
        visible[oy:oy + H, ox:ox + W] = seen
        info[n] = (window.sum() if variant == "all_from_frame" else obj.sum(), window.sum(), (inside & (dt > 0)).sum(), seen.sum())
        box[n] = corners(obj, ox, oy) + corners(visible, ox, oy)
        byte = inside.astype(np.uint8) * CLS_OBJECT + seen.astype(np.uint8) * CLS_VISIBLE
        cls[n] = byte.reshape(W, H) if variant == "row_major" else byte.T
    return cls, info, box, status


# ------------------------------------------------------------------------------------------------ the run lists
def transitions(flat, variant=None, chunk=CHUNK):
    """The positions p with v(p) != v(p - 1), v(-1) = 0, of one instance's bits in column-major order."""
    v = np.asarray(flat, np.uint8)
    before = np.concatenate([[1 if variant == "first_run_ones" else 0], v[:-1]]).astype(np.uint8)
    if variant == "chunk_start_zero":
        before[chunk::chunk] = 0
    return np.flatnonzero(v != before)


def run_lists(flat, variant=None, chunk=CHUNK):
    """-> counts, cum (int64) of one instance: cum = the transitions' positions then H*W, counts its differences."""
    t = transitions(flat, variant, chunk)
    last = (t[-1] if len(t) else 0) if variant == "last_missing" else len(flat)
    cum = np.concatenate([t, [last]]).astype(np.int64)
    return np.diff(np.concatenate([[0], cum])), cum


def bits_of(cls, which):
    cls = np.asarray(cls, np.uint8)
    return ((cls >> which) & 1).reshape(len(cls), -1)


def count_runs(cls, which, variant=None, chunk=CHUNK):
    return np.asarray([len(transitions(v, variant, chunk)) + 1 for v in bits_of(cls, which)], np.int32).reshape(-1)


def write_runs(cls, which, offsets, counts, cum, variant=None, chunk=CHUNK):
    """counts, cum int32[total] are written IN PLACE for every instance whose slice passes the rule -> err (n + 1 of the last
    instance that does not, 0 = none)."""
    err, total = 0, len(counts)
    for n, v in enumerate(bits_of(cls, which)):
        c, s = run_lists(v, variant, chunk)
        lo, hi = int(offsets[n]), int(offsets[n + 1])
        if not (0 <= lo < hi <= total) or hi - lo != len(c):
            err = n + 1
            continue
        counts[lo:hi], cum[lo:hi] = c, s
    return err


def encode_runs(cls, which, variant=None, chunk=CHUNK):
    """-> counts int32 (total,), cum int32 (total,), offsets int32 (N+1,): what gigapose_amd.gtinfo.encode_runs returns."""
    runs = count_runs(cls, which, variant, chunk)
    offsets = np.concatenate([[0], np.cumsum(runs, dtype=np.int64)]).astype(np.int32)
    counts, cum = np.zeros(offsets[-1], np.int32), np.zeros(offsets[-1], np.int32)
    assert write_runs(cls, which, offsets, counts, cum, variant, chunk) == 0
    return counts, cum, offsets


def decode(cum, H, W):
    """One instance's prefix sums -> the dense mask (H,W) by the parity rule of gp_key_walk.h: pixel p = x*H + y is set when
    #{i : cum[i] <= p} is odd."""
    rank = np.searchsorted(np.asarray(cum, np.int64), np.arange(H * W), side="right")
    return (rank & 1).astype(bool).reshape(W, H).T


# ------------------------------------------------------------------------------------------------ GroundTruthInfo.compute on the host
def ray_map(K, H, W):
    k = np.asarray(K, np.float64).reshape(9)
    a = (np.arange(W, dtype=np.float64)[None, :] - k[2]) / k[0]
    b = (np.arange(H, dtype=np.float64)[:, None] - k[5]) / k[4]
    return np.sqrt((a * a + b * b) + 1.0)


def canvas(H, W, margin):
    ox, oy = int(np.ceil(margin * W)), int(np.ceil(margin * H))
    return H + 2 * oy, W + 2 * ox, ox, oy


def draw_on_canvas(vertices, faces, poses, K, H, W, margin, znear=1e-3):
    """poses (N,4,4) f64 drawn from their f32 conversions on the canvas of `margin`, with K whose principal point is moved by the
    frame's origin -> keys (N,Hc,Wc) u64, clipped (N) int32, (ox, oy)."""
    Hc, Wc, ox, oy = canvas(H, W, margin)
    k = np.asarray(K, np.float64).reshape(9).copy()
    k[2], k[5] = k[2] + ox, k[5] + oy
    poses = np.asarray(poses, np.float64)
    vis, clipped = np.zeros((len(poses), Hc, Wc), np.uint64), np.zeros(len(poses), np.int32)
    for n in range(len(poses)):
        xy, vd = raster_ref.project(vertices, poses[n:n + 1].astype(np.float32), k, znear)
        vis[n:n + 1], clipped[n:n + 1] = raster_ref.raster(xy, vd, faces, Hc, Wc)
    return vis, clipped, (ox, oy)


def xywh(c):
    x0, y0, x1, y1 = (int(v) for v in c)
    return [-1, -1, -1, -1] if x1 < x0 else [x0, y0, x1 - x0 + 1, y1 - y0 + 1]


def pose_of(g):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = np.asarray(g["cam_R_m2c"], np.float64).reshape(3, 3), np.asarray(g["cam_t_m2c"], np.float64).reshape(3)
    return P


def compute(models, cameras, gts, delta=15.0, margin=1.0, znear=1e-3, masks=False, variant=None):
    """GroundTruthInfo(models, cameras, delta, margin, znear).compute(gts, masks) on the host, image by image -> {(scene_id, im_id):
    [per instance the dict of the issue]}; with masks also "cls", the instance's bytes (W,H)."""
    out = {}
    for key, listed in gts.items():
        cam = cameras[key]
        depth = None if cam.get("depth") is None else np.asarray(cam["depth"], np.float32)
        H, W = depth.shape if depth is not None else cam["size"]
        rows = []
        for g in listed:
            m = models[int(g["obj_id"])]
            vis, clipped, origin = draw_on_canvas(m["vertices"], m["faces"], pose_of(g)[None], cam["cam_K"], H, W, margin, znear)
            if clipped.any():
                raise ValueError("a ground truth drops a triangle")
            cls, info, box, _ = classify(vis, origin, None if depth is None else depth[None], [0], ray_map(cam["cam_K"], H, W)[None], [0], delta, variant)
            a, _, valid, visib = (int(v) for v in info[0])
            row = dict(px_count_all=a, px_count_valid=valid, px_count_visib=visib, visib_fract=visib / a if a else 0.0,
                       bbox_obj=xywh(box[0, :4]), bbox_visib=xywh(box[0, 4:]))
            if masks:
                row["cls"] = cls[0]
                for name, which in (("mask", 0), ("mask_visib", 1)):
                    row[name] = {"size": [int(H), int(W)], "counts": run_lists(bits_of(cls, which)[0], variant)[0].tolist()}
            rows.append(row)
        out[key] = rows
    return out
