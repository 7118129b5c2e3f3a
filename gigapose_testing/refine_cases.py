"""Inputs for the tests of depth refinement (gigapose_amd/refine.py, gigapose_testing/refine_ref.py), shared by the CPU and the GPU
suite: the small scene the convergence bars are stated on (three_boxes in front of a wall, depths rounded to integers as a depth
PNG holds them), pixels on which every operation of the accumulation is exact together with their reading in rational
arithmetic, and planted rows of sums for the step."""
import functools
from fractions import Fraction

import numpy as np

from . import meshes, raster_ref, refine_ref

H, W = 96, 128
K = np.asarray([114.48, 0.0, 64.0, 0.0, 114.71, 48.0, 0.0, 0.0, 1.0])
SCALE = 120.0
GATE = 0.25 * SCALE
WALL = 520.0
ITERS = 12
TOL = 1e-6
STEP = dict(min_points=32, min_pivot=1e-3, damping=0.0, tol2=TOL * TOL)      # DepthRefiner squares its tol


def rot(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    X = np.asarray([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(t) * X + (1.0 - np.cos(t)) * (X @ X)


def rigid(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


GT = rigid(rot([1, 2, 3], 35) @ rot([0, 1, 0], 20), (10.0, -5.0, 400.0))
GT2 = rigid(rot([2, 1, -1], 40) @ rot([1, 0, 0], 30), (-14.0, 6.0, 380.0))     # like GT it shows faces of three directions


def moved(gt, axis, degrees, offset):
    """The pose `gt` turned about the object's origin (in camera axes) and shifted."""
    return rigid(rot(axis, degrees) @ gt[:3, :3], gt[:3, 3] + np.asarray(offset, np.float64))


def starts(gt=GT):
    return np.stack([moved(gt, [2, -1, 1], a, o) for a, o in ((3, (2, -2, 5)), (8, (5, 4, -12)), (15, (8, -8, 20)))])


def wrong_starts(gt=GT):
    return np.stack([moved(gt, [0, 0, 1], 90, (0, 0, 0)), moved(gt, [1, 0, 0], 180, (0, 0, 0)), moved(gt, [0, 1, 0], 90, (0, 0, 0))])


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f, _ = meshes.three_boxes(60.0) if name == "boxes" else meshes.icosphere(2, 50.0)
    v.setflags(write=False), f.setflags(write=False)
    return v, f


def draw(vertices, faces, pose, k=K, h=H, w=W):
    xy, vd = raster_ref.project(vertices, np.asarray(pose, np.float64)[None].astype(np.float32), k, 1e-3)
    vis, _ = raster_ref.raster(xy, vd, faces, h, w)
    return vis[0]


def depth_of(vis, wall=WALL, rounded=True):
    z = (vis >> np.uint64(32)).astype(np.uint32).view(np.float32)
    d = np.where(vis != raster_ref.EMPTY_KEY, z, np.float32(wall)).astype(np.float32)
    return np.rint(d) if rounded else d


@functools.lru_cache(maxsize=None)
def sensor_depth(name, which=0, rounded=True):
    """(H,W) f32: the object `name` at GT (which = 0) or GT2 (1) in front of the wall."""
    d = depth_of(draw(*mesh(name), (GT, GT2)[which]), rounded=rounded)
    d.setflags(write=False)
    return d


def deviation(vertices, pose, gt=GT):
    """The largest distance between a vertex under `pose` and under `gt`."""
    x = np.asarray(vertices, np.float64)
    return float(np.linalg.norm((x @ pose[:3, :3].T + pose[:3, 3]) - (x @ gt[:3, :3].T + gt[:3, 3]), axis=1).max())


def whole_frame(n, h=H, w=W):
    return np.tile(np.asarray([0, 0, w - 1, h - 1], np.int32), (n, 1))


@functools.lru_cache(maxsize=None)
def run(name, which_starts, variant=None, min_pivot=1e-3, iters=ITERS, rounded=True):
    """The restatement's loop on the scene: `which_starts` is "right" or "wrong".  Cached: several tests read one run."""
    v, f = mesh(name)
    p = starts() if which_starts == "right" else wrong_starts()
    n = len(p)
    step = dict(STEP, min_pivot=min_pivot)
    return refine_ref.refine(v, f, p, np.tile(K, (n, 1)), sensor_depth(name, 0, rounded)[None], np.zeros(n, np.int32), whole_frame(n), np.full(n, GATE),
                             np.full(n, SCALE), iters, step["min_points"], step["min_pivot"], step["damping"], step["tol2"], H, W, variant=variant)


def quality(out):
    """inliers / covered and the rms in model units of each pair of a run."""
    s = out["sums"]
    with np.errstate(all="ignore"):
        ratio = s[:, refine_ref.COUNT] / s[:, refine_ref.COVERED]
        rms = SCALE * np.sqrt(s[:, refine_ref.EE] * 2.0 ** -36 / s[:, refine_ref.COUNT])
    return ratio, rms


# ------------------------------------------------------------------------------------------------ pixels of exact arithmetic
EXACT_K = np.asarray([128.0, 0.5, 64.0, 0.0, 64.0, 48.0, 0.0, 0.0, 1.0])
EXACT_SCALE, EXACT_GATE = 128.0, 6.5
EXACT_NORMALS = np.asarray([(1, 1, 0), (0, 2, -2), (4, 0, 0), (0, 0, -1), (2, 0, 2), (0, -4, 4)], np.float64)   # m.m a power of two
EXACT_POSE = rigid([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], (3.0, -2.0, 300.0))             # a signed permutation, integer translation


def exact_pixels():
    """40 pixels whose every operation up to the terms is exact in float64 (dyadic intrinsics with few bits, depths with four
    fractional bits, normals of integer components with m.m a power of two, a power-of-two scale): keys, dm, px, py.  Pixel 0 sits
    EXACTLY on the gate, pixel 1 the next f32 above it; pixel 2 is uncovered, pixel 3 has no measurement."""
    rs = np.random.RandomState(5)
    n = 40
    px, py = rs.randint(0, W, n), rs.randint(0, H, n)
    zr = (280.0 + rs.randint(0, 16 * 40, n) / 16.0).astype(np.float32)
    dm = (zr.astype(np.float64) + rs.randint(-16 * 10, 16 * 10 + 1, n) / 16.0).astype(np.float32)
    face = rs.randint(0, len(EXACT_NORMALS), n)
    zr[0], dm[0] = 300.0, 306.5
    zr[1], dm[1] = 300.0, np.nextafter(np.float32(306.5), np.float32(400))
    dm[3] = 0.0
    keys = (zr.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)
    keys[2] = raster_ref.EMPTY_KEY
    return keys, dm, px, py


def rational_sums(keys, dm, px, py, c=EXACT_NORMALS, pose=EXACT_POSE, k=EXACT_K, gate=EXACT_GATE, scale=EXACT_SCALE):
    """The header's definitions read in rational arithmetic, pixel by pixel -> the 30 sums as Python integers."""
    Fr = Fraction
    sums = [0] * 30
    R = [[Fr(float(x)) for x in row[:3]] for row in pose[:3]]
    t = [Fr(float(row[3])) for row in pose[:3]]
    k = [Fr(float(x)) for x in k]
    for key, d, x, y in zip(keys.tolist(), dm.tolist(), px.tolist(), py.tolist()):
        if key == 2 ** 64 - 1:
            continue
        sums[28] += 1
        zr = Fr(float(np.asarray([key >> 32], np.uint32).view(np.float32)[0]))
        f = key & 0xFFFFFFFF
        if f >= len(c) or not (np.isfinite(d) and d > 0):
            continue
        r = Fr(float(d)) - zr
        cf = [Fr(float(v)) for v in c[f]]
        m = [sum(R[i][j] * cf[j] for j in range(3)) for i in range(3)]
        mm = sum(v * v for v in m)
        if abs(r) > Fr(gate) or mm == 0:
            continue
        b = (Fr(y) - k[5]) / k[4]
        a = ((Fr(x) - k[2]) - k[1] * b) / k[0]
        q = [a * zr, b * zr, zr]
        dd = [r * a, r * b, r]
        yv = [(q[i] - t[i]) / Fr(scale) for i in range(3)]
        g = [yv[1] * m[2] - yv[2] * m[1], yv[2] * m[0] - yv[0] * m[2], yv[0] * m[1] - yv[1] * m[0]] + m
        e = sum(m[i] * dd[i] for i in range(3)) / Fr(scale)
        terms = [g[i] * g[j] / mm for i, j in refine_ref.PAIRS] + [g[i] * e / mm for i in range(6)] + [e * e / mm]
        assert sum(v * v for v in yv) <= 16 and all(abs(v) <= 16 for v in terms)
        sums[29] += 1
        for o, v in enumerate(terms):
            sums[o] += round(v * 2 ** 36)                   # Fraction.__round__: half to even
    return sums


# ------------------------------------------------------------------------------------------------ planted rows of sums
def sums_row(A, rhs, count, ee=0.0, covered=None):
    """A (6,6), rhs (6,) of multiples of 2^-36 -> one row of 32 int64."""
    row = np.zeros(32, np.int64)
    for o, (i, j) in enumerate(refine_ref.PAIRS):
        row[o] = int(round(float(A[i][j]) * 2.0 ** 36))
    for i in range(6):
        row[refine_ref.RHS + i] = int(round(float(rhs[i]) * 2.0 ** 36))
    row[refine_ref.EE], row[refine_ref.COUNT] = int(round(ee * 2.0 ** 36)), count
    row[refine_ref.COVERED] = count if covered is None else covered
    return row


def integer_ldl(j_bad=None, seed=0):
    """A = L D L^T of small integers (every operation of the factorisation is exact), D positive but D[j_bad] = 0."""
    rs = np.random.RandomState(100 + seed)
    L = np.tril(rs.randint(-2, 3, (6, 6)), -1).astype(np.float64) + np.eye(6)
    D = rs.randint(1, 9, 6).astype(np.float64)
    if j_bad is not None:
        D[j_bad] = 0.0
    return L @ np.diag(D) @ L.T, L, D


def planted_sums():
    """Rows for the step, with the state each must end in: a solvable system with a small step (converged at tol2 = 1e-4), one
    with a large step, too few points, a zero pivot at each of the six positions, and a solvable one for a pair that is stopped
    already.  -> sums (11,32), expected bits (11,), the initial state (11,)."""
    A, _, _ = integer_ldl()
    rows = [sums_row(A * 50, np.asarray([1, -2, 1, 3, -1, 2]) * 2.0 ** -8, 500, 0.25),
            sums_row(A * 50, np.asarray([40, -25, 30, 90, -60, 20], np.float64), 500, 0.5),
            sums_row(A * 50, np.asarray([1, 1, 1, 1, 1, 1], np.float64), 31, 0.5)]
    want = [refine_ref.CONVERGED, 0, refine_ref.FEW]
    for j in range(6):
        rows.append(sums_row(integer_ldl(j, j + 1)[0], np.ones(6), 100))
        want.append(refine_ref.DEGENERATE)
    rows.append(rows[1].copy())
    want.append(refine_ref.FEW)
    rows.append(rows[1].copy())
    want.append(refine_ref.CLIPPED)
    state = np.zeros(len(rows), np.int32)
    state[9] = refine_ref.FEW
    clipped = np.zeros(len(rows), np.int32)
    clipped[10] = 3
    return np.stack(rows), np.asarray(want, np.int32), state, clipped
