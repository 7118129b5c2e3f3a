"""Deterministic test meshes for the renderer (gigapose_amd/render.py, gigapose_testing/raster_ref.py): vertices f32 (V,3), faces
int32 (F,3), colours u8 (V,3); and their UV-mapped variants for the textured renderer (gigapose_amd/texture.py,
gigapose_testing/texture_ref.py): vertices, faces, corner_uv f32 (F,3,2).  Nothing here is random unless a seed is passed."""
import numpy as np


def icosphere(level=2, radius=1.0):
    """An icosahedron subdivided `level` times and pushed to the sphere: 20 * 4**level faces (2: 320, 3: 1280, 5: 20480).
    Outward winding.  The colour of a vertex is its direction mapped to [32, 223]."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(a, np.float64) / np.linalg.norm(a) for a in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.asarray(v)
    colours = np.rint(127.5 + 95.5 * v).astype(np.uint8)
    return (v * radius).astype(np.float32), np.asarray(f, np.int32), colours


_BOX_FACES = [((0, 3, 2, 1), "-z"), ((4, 5, 6, 7), "+z"), ((0, 1, 5, 4), "-y"), ((3, 7, 6, 2), "+y"), ((0, 4, 7, 3), "-x"),
              ((1, 2, 6, 5), "+x")]


def box(size=(1.0, 1.0, 1.0), centre=(0.0, 0.0, 0.0), face_colours=None):
    """An axis-aligned box: 6 quads of their own 4 vertices (so a face has ONE colour), 12 triangles, outward winding.
    face_colours: (6,3) in the order -z +z -y +y -x +x; the default gives six distinct colours."""
    s, c = np.asarray(size, np.float64) / 2, np.asarray(centre, np.float64)
    corners = np.asarray([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float64) * s + c
    if face_colours is None:
        face_colours = [(230, 40, 40), (40, 230, 40), (40, 40, 230), (230, 230, 40), (230, 40, 230), (40, 230, 230)]
    v, f, col = [], [], []
    for (quad, _), colour in zip(_BOX_FACES, face_colours):
        o = len(v)
        v += [corners[i] for i in quad]
        f += [(o, o + 1, o + 2), (o, o + 2, o + 3)]
        col += [colour] * 4
    return np.asarray(v, np.float32), np.asarray(f, np.int32), np.asarray(col, np.uint8)


def merge(parts):
    v, f, c, o = [], [], [], 0
    for pv, pf, pc in parts:
        v.append(pv)
        f.append(pf + o)
        c.append(pc)
        o += len(pv)
    return np.concatenate(v), np.concatenate(f).astype(np.int32), np.concatenate(c)


def three_boxes(scale=1.0):
    """An object without any symmetry: three boxes of different size and colour family on the +x, +y and +z axes, touching a
    small cube at the origin.  Every quad has its own colour (24 distinct colours + the cube's 6)."""
    def shades(base):
        return [tuple(int(min(255, b * k // 8)) for b in base) for k in (8, 7, 6, 5, 4, 3)]

    parts = [box((0.4, 0.4, 0.4), (0, 0, 0), shades((200, 200, 200))),
             box((1.2, 0.3, 0.3), (0.8, 0, 0), shades((255, 64, 32))),
             box((0.35, 0.8, 0.35), (0, 0.6, 0), shades((32, 255, 64))),
             box((0.25, 0.25, 0.5), (0, 0, 0.45), shades((48, 96, 255)))]
    v, f, c = merge(parts)
    return (v * np.float32(scale)).astype(np.float32), f, c


def convex_polygon(n=7, radius=1.0, z=0.0):
    """A regular n-gon in the plane z = const, fan-triangulated about vertex 0; the colours run round the rim."""
    a = 2 * np.pi * np.arange(n) / n
    v = np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], axis=1).astype(np.float32)
    f = np.asarray([(0, i, i + 1) for i in range(1, n - 1)], np.int32)
    c = np.stack([np.rint(127.5 + 127.5 * np.cos(a)), np.rint(127.5 + 127.5 * np.sin(a)), np.full(n, 128.0)], axis=1).astype(np.uint8)
    return v, f, c


# ------------------------------------------------------------------------------------------------ UV-mapped shapes
def uv_quad(size=(1.0, 1.0), z=0.0, uv_min=(0.0, 0.0), uv_max=(1.0, 1.0)):
    """A rectangle in the plane z = const, two triangles.  Seen with the identity rotation (x right, y down) the texture stands
    upright: the vertex at (-w/2, -h/2), the top-left of the image, carries (u_min, v_max).  uv_min / uv_max beyond [0, 1] repeat
    the texture."""
    w, h = size[0] / 2.0, size[1] / 2.0
    (u0, v0), (u1, v1) = uv_min, uv_max
    v = np.asarray([(-w, -h, z), (w, -h, z), (w, h, z), (-w, h, z)], np.float32)
    uv = np.asarray([(u0, v1), (u1, v1), (u1, v0), (u0, v0)], np.float32)
    f = np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)
    return v, f, uv[f]


BOX_ATLAS = {"-z": (0, 0), "+z": (1, 0), "-y": (2, 0), "+y": (3, 0), "-x": (0, 1), "+x": (1, 1)}     # cell (column, row) of 4 x 2, row 0 = v < 1/2


def uv_box(size=(1.0, 1.0, 1.0), centre=(0.0, 0.0, 0.0), shared=True):
    """box() with an atlas: face `name` fills cell BOX_ATLAS[name] of a 4 x 2 grid (so -z, +z lie in the texture's bottom-left
    quadrant, -y, +y in the bottom-right one, -x, +x in the top-left one; the top-right quadrant is unused).  shared=True: the 8
    corners are the vertices, so every vertex carries three different UVs -- seams that only per-corner UVs can express.
    shared=False: 24 vertices, one UV each (corner_uv is then vertex_uv[faces]).  Same faces in the same order either way."""
    s, c = np.asarray(size, np.float64) / 2, np.asarray(centre, np.float64)
    corners = np.asarray([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float64) * s + c
    v, f, uv = [], [], []
    for quad, name in _BOX_FACES:
        cx, cy = BOX_ATLAS[name]
        cell = [((cx + a) / 4.0, (cy + b) / 2.0) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
        if shared:
            idx = list(quad)
        else:
            idx = list(range(len(v), len(v) + 4))
            v += [corners[i] for i in quad]
        for tri in ((0, 1, 2), (0, 2, 3)):
            f.append([idx[k] for k in tri])
            uv.append([cell[k] for k in tri])
    v = corners if shared else np.asarray(v)
    return v.astype(np.float32), np.asarray(f, np.int32), np.asarray(uv, np.float32)


def uv_icosphere(level=2, radius=1.0):
    """icosphere() with a longitude / latitude map: u = longitude / 2 pi + 1/2, v = latitude / pi + 1/2.  A face that straddles
    the date line gets 1 added to its corners' u on the low side, so its UVs run beyond 1: per-corner, and repeat wrapping."""
    v, f, _ = icosphere(level, 1.0)
    d = v.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u = np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5
    w = np.arcsin(np.clip(d[:, 2], -1, 1)) / np.pi + 0.5
    cu, cw = u[f], w[f]
    wide = (cu.max(axis=1) - cu.min(axis=1)) > 0.5
    cu = np.where(wide[:, None] & (cu < 0.5), cu + 1.0, cu)
    return (v * np.float32(radius)).astype(np.float32), f, np.stack([cu, cw], axis=2).astype(np.float32)


# ------------------------------------------------------------------------------------------------ polygons in screen coordinates
MAX_POLY = 8


def screen_polygon(rs, H, W, on_centres):
    """A strictly convex polygon of 3..8 vertices inside an H x W frame, int64 (n,2) in units of 1/256 pixel (`on_centres`:
    every vertex on a pixel centre), counter-clockwise in (x, y), and an interior point c (1,2) for a fan about it: the
    centroid, snapped to the same grid."""
    unit = 256 if on_centres else 1
    while True:
        n = int(rs.randint(3, MAX_POLY + 1))
        cx, cy = rs.uniform(0.3, 0.7) * W, rs.uniform(0.3, 0.7) * H
        rx, ry = rs.uniform(0.15, 0.5) * W, rs.uniform(0.15, 0.5) * H
        a = np.sort(rs.uniform(0, 2 * np.pi, n))
        p = np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], axis=1)
        p = (np.rint(p * 256 / unit) * unit).astype(np.int64)
        c = (np.rint(p.mean(axis=0) / unit) * unit).astype(np.int64)
        q, r = np.roll(p, -1, axis=0), np.roll(p, -2, axis=0)
        turn = (q[:, 0] - p[:, 0]) * (r[:, 1] - q[:, 1]) - (q[:, 1] - p[:, 1]) * (r[:, 0] - q[:, 0])
        side = (q[:, 0] - p[:, 0]) * (c[1] - p[:, 1]) - (q[:, 1] - p[:, 1]) * (c[0] - p[:, 0])
        if (turn > 0).all() and (side > 0).all():       # strictly convex, and the snapped centroid strictly inside
            return p, c[None]


def fan_faces(n, about_centre):
    """Faces of a fan over polygon vertices 0..n-1: about vertex 0, or about the extra vertex n (the interior point)."""
    if about_centre:
        return np.asarray([(n, i, (i + 1) % n) for i in range(n)], np.int32)
    return np.asarray([(0, i, i + 1) for i in range(1, n - 1)], np.int32)


def padded_polygon(p, c):
    """(MAX_POLY + 1, 2) int32: the polygon, its last vertex repeated up to MAX_POLY, then the interior point -- so that
    fan_faces(MAX_POLY, ...) draws a polygon of any size (the repeated vertices give zero-area triangles)."""
    pad = np.repeat(p[-1:], MAX_POLY - len(p), axis=0)
    return np.concatenate([p, pad, c]).astype(np.int32)
