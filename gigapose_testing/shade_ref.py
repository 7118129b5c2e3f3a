"""The two entry points of libgigapose_shade.so restated in numpy from the description in include/gigapose_shade.h (the arithmetic
there is the contract): integer sums of quantised face cross products, float64 in the written order, numpy.sqrt for the
correctly rounded root.  The GPU tests compare the kernels with this bit for bit.

`wrong` selects a deliberately wrong shader; only None is the contract.  tests/test_shade_host.py uses the others to show that
each of its checks can fail."""
import numpy as np

from . import raster_ref

RANGE, NO_NORMAL = 1, 2
SMOOTH, FLAT = 0, 1
MAX_LIGHTS = 16
MAX_QUANTUM = 2.0 ** 40
WRONG = ("no_flip", "unnormalised", "falloff_1_over_d", "object_lights", "screen_weights", "wrong_key_half", "truncate_encode")


def _check(wrong):
    if wrong is not None and wrong not in WRONG:
        raise ValueError(f"wrong must be None or one of {WRONG}")


def face_cross(vertices, faces):
    """(F,3) float64: gpf_face_normals' c from the stored vertex order (the indices must be in range)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        u, w = p1 - p0, p2 - p0
        return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def vertex_normals(vertices, faces, unit, wrong=None):
    """vertices (V,3) f32, faces (F,3) -> acc (V,3) int64, flags (V,) int32, normals (V,3) float64."""
    _check(wrong)
    V = len(vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < V)).all(axis=1)]
    acc, flags = np.zeros((V, 3), np.int64), np.zeros(V, np.int32)
    with np.errstate(all="ignore"):
        q = np.rint(face_cross(vertices, f) * np.float64(unit))
        ok = (np.abs(q) <= MAX_QUANTUM).all(axis=1)
        for k in range(3):
            np.add.at(acc, f[ok, k], q[ok].astype(np.int64))
            np.bitwise_or.at(flags, f[~ok, k], np.int32(RANGE))
        a = acc.astype(np.float64)
        aa = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        none = (aa == 0.0) | (flags != 0)
        n = a / np.sqrt(np.where(none, 1.0, aa))[:, None]
    if wrong == "unnormalised":
        n = a.copy()
    n[none] = 0.0
    flags[none] |= NO_NORMAL
    return acc, flags, n


def shade(vis, xy, depth, faces, colours, vertices, normals, poses, K, lights, ambient, decode, encode, mode, wrong=None, with_E=False):
    """-> rgba (N,H,W,4) u8, zdepth (N,H,W) f32, unlit (N,) int32 [, E (N,H,W) float64, NaN where nothing is drawn]."""
    _check(wrong)
    faces = np.asarray(faces)
    col = np.asarray(colours, np.uint8).astype(np.float64)
    P = np.asarray(poses, np.float32).astype(np.float64)
    k = np.asarray(K, np.float32).astype(np.float64).reshape(9)
    lights = np.asarray(lights, np.float64).reshape(-1, 4)
    decode, encode = np.asarray(decode, np.float64), np.asarray(encode, np.uint8)
    T = len(encode)
    assert len(lights) <= MAX_LIGHTS and decode.shape == (256,) and 256 <= T <= 65536 and mode in (SMOOTH, FLAT)
    ambient, top = np.float64(ambient), np.float64(T - 1)
    N, H, W = np.asarray(vis).shape
    rgba, zdepth, unlit = np.zeros((N, H, W, 4), np.uint8), np.zeros((N, H, W), np.float32), np.zeros(N, np.int32)
    Emap = np.full((N, H, W), np.nan)
    with np.errstate(all="ignore"):
        for n, f, tri, py, px, e, _, r, z in raster_ref.drawn(vis, xy, depth, faces, 32 if wrong == "wrong_key_half" else 0):
            lit = lights.copy()
            if wrong == "object_lights":
                lit[:, :3] = lights[:, :3] @ P[n, :3, :3].T + P[n, :3, 3]
            t, q = raster_ref.weights(e, [1.0, 1.0, 1.0] if wrong == "screen_weights" else r)
            if mode == FLAT:
                g = [np.full(len(px), c) for c in face_cross(vertices, faces[f][None])[0]]
            else:
                n0, n1, n2 = (np.asarray(normals, np.float64)[i] for i in tri[0])
                g = [(t[0] * n0[j] + t[1] * n1[j]) + t[2] * n2[j] for j in range(3)]
            m = [(P[n, row, 0] * g[0] + P[n, row, 1] * g[1]) + P[n, row, 2] * g[2] for row in range(3)]
            zd = z.astype(np.float64)
            yn = (py.astype(np.float64) - k[5]) / k[4]
            xn = ((px.astype(np.float64) - k[2]) - k[1] * yn) / k[0]
            p = [xn * zd, yn * zd, zd]
            s = (m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]
            if wrong != "no_flip":
                m = [np.where(s > 0, -mj, mj) for mj in m]
            mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
            usable = (mm > 0) & (mm < np.inf)
            unlit[n] += int((~usable).sum())
            E = np.full(len(px), ambient)
            for l in range(len(lit)):
                d = [lit[l, j] - p[j] for j in range(3)]
                dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                md = (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2]
                if wrong == "falloff_1_over_d":
                    add = (lit[l, 3] * md) / (np.sqrt(mm * dd) * np.sqrt(dd))
                else:
                    add = (lit[l, 3] * md) / (np.sqrt(mm * dd) * dd)
                E = np.where(usable & (md > 0) & (dd > 0), E + add, E)
            Emap[n, py, px] = E
            for c in range(3):
                c0, c1, c2 = (col[i, c] for i in tri[0])
                b = raster_ref.colour_bytes(t, q, c0, c1, c2)
                b = np.where(np.isnan(b), 0.0, b).astype(np.int64)
                w = (decode[b] * E) * top
                w = np.floor(w if wrong == "truncate_encode" else w + 0.5)
                i = np.where(w >= top, top, np.where(w > 0, w, 0.0)).astype(np.int64)
                rgba[n, py, px, c] = encode[i]
            rgba[n, py, px, 3] = 255
            zdepth[n, py, px] = z
    return (rgba, zdepth, unlit, Emap) if with_E else (rgba, zdepth, unlit)


def render(vertices, faces, colours, normals, poses, K, H, W, znear, lights, ambient, decode, encode, mode, wrong=None, with_E=False):
    xy, depth = raster_ref.project(vertices, poses, K, znear)
    vis, clipped = raster_ref.raster(xy, depth, faces, H, W)
    out = shade(vis, xy, depth, faces, colours, vertices, normals, poses, K, lights, ambient, decode, encode, mode, wrong, with_E)
    res = dict(xy=xy, vdepth=depth, vis=vis, clipped=clipped, rgba=out[0], depth=out[1], unlit=out[2])
    if with_E:
        res["E"] = out[3]
    return res


# ------------------------------------------------------------------------------------------------ cases both test files use
def fan(count=70):
    a = 2 * np.pi * np.arange(count) / count
    ring = np.stack([np.rint(100 * np.cos(a)), np.rint(100 * np.sin(a)), np.zeros(count)], axis=1)
    v = np.concatenate([[(0, 0, 30)], ring]).astype(np.float32)
    f = np.asarray([(0, 1 + i, 1 + (i + 1) % count) for i in range(count)], np.int32)
    return v, f


def guard_cases():
    """name -> (vertices, faces, unit, expected flags)."""
    big = float(2 ** 20)
    tri = np.asarray([(0, 1, 2)], np.int32)
    nan = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (np.nan, 0, 0), (5, 5, 5)], np.float32)
    return {
        "just inside: q = 2^40": (np.asarray([(0, 0, 0), (big, 0, 0), (0, big, 0)], np.float32), tri, 1.0, [0, 0, 0]),
        "just beyond: q = 2^40 + 2^20": (np.asarray([(0, 0, 0), (big, 0, 0), (0, big + 1, 0)], np.float32), tri, 1.0, [3, 3, 3]),
        "beyond through the unit": (np.asarray([(0, 0, 0), (big, 0, 0), (0, big, 0)], np.float32), tri, 2.0, [3, 3, 3]),
        "a NaN vertex": (nan, np.asarray([(0, 1, 2), (1, 2, 3)], np.int32), 1.0, [0, 3, 3, 3, 2]),
        "an infinite product": (np.asarray([(0, 0, 0), (3e38, 0, 0), (0, 3e38, 0)], np.float32), tri, 2.0 ** 900, [3, 3, 3]),
        "an unused vertex": (np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (7, 7, 7)], np.float32), tri, 4.0, [0, 0, 0, 2]),
        "faces that cancel": (np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32),
                              np.asarray([(0, 1, 2), (0, 2, 1), (1, 2, 3)], np.int32), 4.0, [2, 0, 0, 0]),
        "an index out of range": (np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32), np.asarray([(0, 1, 3), (0, -1, 2), (0, 1, 2)], np.int32), 4.0,
                                  [0, 0, 0]),
        "no face": (np.asarray([(1, 2, 3)], np.float32), np.zeros((0, 3), np.int32), 1.0, [2]),
    }
