"""The three stages of libgigapose_render.so restated in numpy from the description in include/gigapose_render.h (the arithmetic
there is the contract): int64 edge functions on 1/256-pixel coordinates, the top-left rule, float64 interpolation in the
written order, one rounding to f32 for the key.  The GPU tests compare the kernels with this bit for bit.

It loops per (view, triangle) over the triangle's bounding box, vectorised inside the box: usable up to a few thousand
triangles per view.  `rule` selects the coverage rule; only "top_left" is the contract, the others are deliberately wrong
rasterisers that tests/test_render_host.py uses to show that its partition check can fail."""
import numpy as np

BAD_COORD = np.int32(-2 ** 31)
MAX_PIXEL = 16384.0
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
RULES = ("top_left", "closed", "open", "ties_on_edge0", "ties_dx_or_dy")


def project(vertices, poses, K, znear):
    """vertices (V,3) f32, poses (N,4,4) f32, K 9 floats -> xy (N,V,2) int32 in 1/256 pixel, depth (N,V) f32."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    P = np.asarray(poses, np.float32).astype(np.float64)
    k = np.asarray(K, np.float32).astype(np.float64).reshape(9)
    x, y, z = v[None, :, 0], v[None, :, 1], v[None, :, 2]

    def row(r):
        return ((P[:, r, 0, None] * x + P[:, r, 1, None] * y) + P[:, r, 2, None] * z) + P[:, r, 3, None]

    with np.errstate(all="ignore"):
        X, Y, Z = row(0), row(1), row(2)
        u = ((k[0] * X + k[1] * Y) + k[2] * Z) / Z
        w = ((k[3] * X + k[4] * Y) + k[5] * Z) / Z
        depth = Z.astype(np.float32)
        good = (depth >= np.float32(znear)) & (np.abs(u) <= MAX_PIXEL) & (np.abs(w) <= MAX_PIXEL)
        su = np.where(good, np.rint(np.where(good, u, 0.0) * 256.0), float(BAD_COORD))
        sw = np.where(good, np.rint(np.where(good, w, 0.0) * 256.0), float(BAD_COORD))
    return np.stack([su, sw], axis=-1).astype(np.int32), depth


def _accept(e, dx, dy, rule, edge):
    if rule == "top_left":
        tie = dy < 0 or (dy == 0 and dx > 0)
    elif rule == "closed":
        tie = True
    elif rule == "open":
        tie = False
    elif rule == "ties_on_edge0":
        tie = edge == 0
    elif rule == "ties_dx_or_dy":
        tie = dy < 0 or dx > 0
    else:
        raise ValueError(f"rule must be one of {RULES}")
    return (e > 0) | ((e == 0) & tie)


def setup(xy_n, faces, f, V):
    """The triangle f of one view: None when dropped (second value: clipped?), else ordered indices and int coordinates."""
    idx = [int(i) for i in faces[f]]
    if any(i < 0 or i >= V for i in idx):
        return None, True
    pts = [(int(xy_n[i, 0]), int(xy_n[i, 1])) for i in idx]
    if any(p[0] == int(BAD_COORD) for p in pts):
        return None, True
    (x0, y0), (x1, y1), (x2, y2) = pts
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if area == 0:
        return None, False
    if area < 0:
        idx[1], idx[2] = idx[2], idx[1]
        pts[1], pts[2] = pts[2], pts[1]
        area = -area
    return (idx, pts, area), False


def edge_values(pts, px, py):
    """px, py: int64 arrays of pixel indices -> e0, e1, e2 (int64) and the (dx, dy) of the three edges."""
    X, Y = px * 256, py * 256
    out, dirs = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = pts[b][0] - pts[a][0], pts[b][1] - pts[a][1]
        out.append(dx * (Y - pts[a][1]) - dy * (X - pts[a][0]))
        dirs.append((dx, dy))
    return out, dirs


def box(pts, H, W):
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    bx0, bx1 = max(-(-min(xs) // 256), 0), min(max(xs) // 256, W - 1)
    by0, by1 = max(-(-min(ys) // 256), 0), min(max(ys) // 256, H - 1)
    return bx0, by0, bx1, by1


def box_pixels(xy_n, faces, f, H, W):
    """The pixel count of the clamped bounding box of triangle f (0: dropped or empty): what the small / large split looks at."""
    tri, _ = setup(xy_n, np.asarray(faces), f, len(xy_n))
    if tri is None:
        return 0
    bx0, by0, bx1, by1 = box(tri[1], H, W)
    return max(bx1 - bx0 + 1, 0) * max(by1 - by0 + 1, 0)


def _covered(tri, H, W, rule):
    idx, pts, area = tri
    bx0, by0, bx1, by1 = box(pts, H, W)
    if bx1 < bx0 or by1 < by0:
        return None
    py, px = np.meshgrid(np.arange(by0, by1 + 1, dtype=np.int64), np.arange(bx0, bx1 + 1, dtype=np.int64), indexing="ij")
    e, dirs = edge_values(pts, px, py)
    inside = np.ones(px.shape, bool)
    for k in range(3):
        inside &= _accept(e[k], dirs[k][0], dirs[k][1], rule, k)
    return px[inside], py[inside], [ek[inside] for ek in e]


def coverage(xy_n, faces, H, W, rule="top_left"):
    """How many triangles cover each pixel: (H,W) int32.  xy_n (V,2) int32."""
    xy_n, faces = np.asarray(xy_n), np.asarray(faces)
    count = np.zeros((H, W), np.int32)
    for f in range(len(faces)):
        tri, _ = setup(xy_n, faces, f, len(xy_n))
        if tri is None:
            continue
        got = _covered(tri, H, W, rule)
        if got is not None:
            np.add.at(count, (got[1], got[0]), 1)
    return count


def raster(xy, depth, faces, H, W, rule="top_left"):
    """xy (N,V,2) int32, depth (N,V) f32, faces (F,3) -> vis (N,H,W) uint64, clipped (N,) int32."""
    xy, depth, faces = np.asarray(xy), np.asarray(depth, np.float32), np.asarray(faces)
    N, V = depth.shape
    vis = np.full((N, H, W), EMPTY_KEY, np.uint64)
    clipped = np.zeros(N, np.int32)
    for n in range(N):
        for f in range(len(faces)):
            tri, clip = setup(xy[n], faces, f, V)
            clipped[n] += clip
            if tri is None:
                continue
            got = _covered(tri, H, W, rule)
            if got is None or not len(got[0]):
                continue
            px, py, e = got
            r = [1.0 / np.float64(depth[n, i]) for i in tri[0]]
            q = (e[0].astype(np.float64) * r[0] + e[1].astype(np.float64) * r[1]) + e[2].astype(np.float64) * r[2]
            z = (np.float64(tri[2]) / q).astype(np.float32)
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            vis[n, py, px] = np.minimum(vis[n, py, px], key)      # a triangle covers a pixel at most once: no duplicate index
    return vis, clipped


def drawn(vis, xy, depth, faces, face_shift=0):
    """What the three resolves (this file's, texture_ref's, shade_ref's) share: per view n and per face f that a covered key of
    the view names, that is < F and that sets up, yields (n, f, tri, py, px, e, dirs, r, z) -- tri as `setup` returns it, the
    pixels (int64) whose key names f, their edge values e[k] with the edges' directions, r[k] = 1 / depth of corner k (apart from
    e, so that a caller can weight differently: the mutants), and the depth z (f32) the keys carry.  face_shift = 32 reads the
    face from the wrong half of the key (a mutant).  vis: uint64, or int64 holding the same bits."""
    vis, xy, depth, faces = np.asarray(vis).view(np.uint64), np.asarray(xy), np.asarray(depth, np.float32), np.asarray(faces)
    V = depth.shape[1]
    face_of = ((vis >> np.uint64(face_shift)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for n in range(vis.shape[0]):
        covered = vis[n] != EMPTY_KEY
        for f in np.unique(face_of[n][covered]):
            tri = setup(xy[n], faces, int(f), V)[0] if f < len(faces) else None
            if tri is None:
                continue
            py, px = np.nonzero(covered & (face_of[n] == f))
            py, px = py.astype(np.int64), px.astype(np.int64)
            e, dirs = edge_values(tri[1], px, py)
            with np.errstate(all="ignore"):
                r = [1.0 / np.float64(depth[n, i]) for i in tri[0]]
            yield n, int(f), tri, py, px, e, dirs, r, (vis[n, py, px] >> np.uint64(32)).astype(np.uint32).view(np.float32)


def weights(e, r):
    """-> [t_0, t_1, t_2], q: t_k = (float64)e_k * r_k, q = (t_0 + t_1) + t_2."""
    t = [e[k].astype(np.float64) * r[k] for k in range(3)]
    return t, (t[0] + t[1]) + t[2]


def colour_bytes(t, q, c0, c1, c2):
    """floor(((t_0 c_0 + t_1 c_1) + t_2 c_2) / q + 1/2), clamped to [0, 255]: float64, not yet a byte (a NaN stays one)."""
    return np.clip(np.floor(((t[0] * c0 + t[1] * c1) + t[2] * c2) / q + 0.5), 0.0, 255.0)


def resolve(vis, xy, depth, faces, colours):
    """-> rgba (N,H,W,4) u8, zdepth (N,H,W) f32."""
    colours = np.asarray(colours, np.uint8).astype(np.float64)
    N, H, W = np.asarray(vis).shape
    rgba = np.zeros((N, H, W, 4), np.uint8)
    zdepth = np.zeros((N, H, W), np.float32)
    for n, _, tri, py, px, e, _, r, z in drawn(vis, xy, depth, faces):
        t, q = weights(e, r)
        for c in range(3):
            rgba[n, py, px, c] = colour_bytes(t, q, *(colours[i, c] for i in tri[0])).astype(np.uint8)
        rgba[n, py, px, 3] = 255
        zdepth[n, py, px] = z
    return rgba, zdepth


def render(vertices, faces, colours, poses, K, H, W, znear):
    xy, depth = project(vertices, poses, K, znear)
    vis, clipped = raster(xy, depth, faces, H, W)
    rgba, zdepth = resolve(vis, xy, depth, faces, colours)
    return dict(xy=xy, vdepth=depth, vis=vis, clipped=clipped, rgba=rgba, depth=zdepth)
