"""The numpy restatement of include/gigapose_dist.h: ADD / ADD-S as integer sums of quantised distances, and the square of the
model diameter as the bit pattern of a double.  Written from the header, not from the kernels: every line is one rounding per
written operation in the written order (numpy never fuses), the root is numpy.sqrt (correctly rounded), the minimum is
numpy.fmin from +inf.  The kernels are held to it bit for bit (tests/test_gpu_dist.py); tests/test_dist_host.py holds it to exact
integer arithmetic.  All pairs are visited in chunks of query points, so V = 2 049 needs a few megabytes.

`variant` selects a deliberately WRONG scorer, for the tests that show the checks reject them."""
import numpy as np

QUERY_CHUNK = 256
BLOCK_ELEMENTS = 1 << 22                 # point pairs held at a time
LIMIT = 2.0 ** 42
BAD_KEY = 2 ** 64 - 1
VARIANTS = ("reversed", "mean_of_squares", "floor", "skip_self", "tile_stop")


def transform(M, vertices):
    """Rows 0..2 of M (4,4) or (N,4,4) applied to vertices (V,3) f32 converted to float64 -> (V,3) or (N,V,3):
    ((M0*x + M1*y) + M2*z) + M3."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    M = np.asarray(M, np.float64)[..., None]
    return np.stack([((M[..., i, 0, :] * x + M[..., i, 1, :] * y) + M[..., i, 2, :] * z) + M[..., i, 3, :] for i in range(3)], axis=-1)


def dist2(a, b):
    """d2 of broadcastable point arrays (..., 3)."""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(queries, points, variant=None, tile=1024):
    """queries (..., Q, 3), points (..., V, 3): for each query the minimum of d2 over the points, from +inf, a NaN candidate never
    taken -> (values (..., Q), index (..., Q) of the first point that reaches it)."""
    queries, points = np.asarray(queries), np.asarray(points)
    single = queries.ndim == 2
    queries, points = queries.reshape((-1,) + queries.shape[-2:]), points.reshape((-1,) + points.shape[-2:])
    N, Q, V = len(queries), queries.shape[1], points.shape[1]
    stop = V if variant != "tile_stop" or V < tile else (V // tile) * tile
    vals, idx = np.empty((N, Q)), np.empty((N, Q), np.int64)
    block = max(1, min(N, BLOCK_ELEMENTS // (min(Q, QUERY_CHUNK) * V)))
    with np.errstate(all="ignore"):
        for n in range(0, N, block):
            for a in range(0, Q, QUERY_CHUNK):
                d2 = dist2(queries[n:n + block, a:a + QUERY_CHUNK, None, :], points[n:n + block, None, :stop, :])
                if variant == "skip_self":
                    i = np.arange(a, min(a + QUERY_CHUNK, Q, stop))
                    d2[:, i - a, i] = np.inf
                m = np.fmin.reduce(d2, axis=2, initial=np.inf)
                vals[n:n + block, a:a + QUERY_CHUNK] = m
                idx[n:n + block, a:a + QUERY_CHUNK] = np.argmax(d2 == m[..., None], axis=2)
    return (vals[0], idx[0]) if single else (vals, idx)


def point_values(vertices, est, gt, symmetric, variant=None, tile=1024):
    """est, gt (N,4,4) -> v (N,V) and, per pair, whether every coordinate of e and g is finite."""
    with np.errstate(all="ignore"):
        e, g = transform(est, vertices), transform(gt, vertices)
        ok = np.isfinite(e).all(axis=(1, 2)) & np.isfinite(g).all(axis=(1, 2))
        if not symmetric:
            return dist2(e, g), ok
        if variant == "reversed":
            return nearest(e, g)[0], ok
        return nearest(g, e, variant, tile)[0], ok


def quantise(v, k, variant=None):
    """v (N,V) -> sums (N,) int64 and the status words (N,) int32."""
    with np.errstate(all="ignore"):
        r = v if variant == "mean_of_squares" else np.sqrt(v)
        s = r * 2.0 ** k
        in_range = s < LIMIT
        q = np.where(in_range, (np.floor if variant == "floor" else np.rint)(np.where(in_range, s, 0.0)), 0.0).astype(np.int64)
    status = np.where((v < np.inf).all(axis=1), 0, 1) | np.where(in_range.all(axis=1), 0, 2)
    return q.sum(axis=1, dtype=np.int64), status.astype(np.int32)     # each q < 2^42, V <= 2^20: the int64 sum is exact


def add_sums(vertices, est, gt, symmetric, k=20, variant=None, tile=1024):
    """-> sums int64 (N,), status int32 (N,).  `k` may be a tuple: -> {k: (sums, status)} from one pass over the point pairs."""
    est, gt = np.asarray(est, np.float64).reshape(-1, 4, 4), np.asarray(gt, np.float64).reshape(-1, 4, 4)
    v, ok = point_values(vertices, est, gt, symmetric, variant, tile)
    out = {}
    for kk in (k if isinstance(k, tuple) else (k,)):
        sums, status = quantise(v, kk, variant)
        out[kk] = (sums, status | np.where(ok, 0, 1).astype(np.int32))
    return out if isinstance(k, tuple) else out[k]


def errors_from_sums(sums, status, V, k):
    """sums / (V * 2^k) with Python integers (a correctly rounded division); +inf where a status bit is set."""
    out = []
    for s, b in zip(np.asarray(sums).tolist(), np.asarray(status).tolist()):
        out.append(np.inf if b else (s / (V << k) if k >= 0 else (s << -k) / V))
    return np.asarray(out, np.float64).reshape(-1)


def add_errors(vertices, est, gt, symmetric, k=20, variant=None, tile=1024):
    sums, status = add_sums(vertices, est, gt, symmetric, k, variant, tile)
    return errors_from_sums(sums, status, len(vertices), k)


def diameter2_key(vertices, variant=None, pad=(0.0, 0.0, 0.0)):
    """-> the key as a Python integer: the bits of max over i < j of d2, all ones if one of them is not below +inf, 0 for V = 1.
    variant "past_end": i <= j <= V, reading the row after the last vertex (`pad` stands for what lies there)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    V = len(v)
    if variant == "past_end":
        v = np.concatenate([v, np.asarray(pad, np.float64)[None]])
    best, bad = 0.0, False
    with np.errstate(all="ignore"):
        for a in range(0, V, QUERY_CHUNK):
            d2 = dist2(v[a:a + QUERY_CHUNK, None, :][:V - a], v[None, :, :])
            i, j = np.arange(a, min(a + QUERY_CHUNK, V))[:, None], np.arange(len(v))[None, :]
            d2 = d2[np.broadcast_to(j >= i if variant == "past_end" else j > i, d2.shape)]
            if d2.size:
                bad |= not bool((d2 < np.inf).all())
                best = max(best, float(np.fmax.reduce(d2)))
    return BAD_KEY if bad else int(np.asarray([best], np.float64).view(np.uint64)[0])


def diameter(vertices):
    key = diameter2_key(vertices)
    if key == BAD_KEY:
        raise ValueError("a vertex is not finite")
    return float(np.sqrt(np.asarray([key], np.uint64).view(np.float64))[0])
