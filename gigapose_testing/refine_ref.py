"""libgigapose_refine.so restated in numpy from the description in include/gigapose_refine.h (the arithmetic there is the
contract): the unnormalised face normals, the per-pixel terms of the point-to-plane normal equations quantised to 2^-36 and
summed as integers, the unpivoted LDL^T, the Cayley step.  The GPU tests compare the kernels with this bit for bit; the loop at
the end (refine) is DepthRefiner.refine over raster_ref's rasteriser.

`variant` selects a deliberately WRONG refiner (tests/test_refine_host.py shows that its checks reject each): None is the
contract."""
import numpy as np

from . import raster_ref

SUMS, RHS, EE, COVERED, COUNT = 32, 21, 27, 28, 29
QUANTUM = 2.0 ** 36
TERM_MAX = 16.0
RANGE, BAD_INDEX, FEW, DEGENERATE, CLIPPED, CONVERGED = 1, 2, 4, 8, 16, 32
STOP = FEW | DEGENERATE | CLIPPED
VARIANTS = ("cross_swapped", "full_omega", "unscaled_t", "camera_origin", "weight_inv_norm", "floor", "strict_gate")
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def face_normals(vertices, faces):
    """vertices (V,3) f32, faces (F,3) -> c (F,3) f64; a vertex index outside [0, V) gives NaN."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    u, w = v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]]
    c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    c[~ok] = np.nan
    return c


def clamp_box(box, H, W):
    x0, y0, x1, y1 = (int(b) for b in box)
    return max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)


def pixel_terms(keys, dm, px, py, c, pose, K, gate, scale, variant=None):
    """The pixels (any shape P...) of ONE pair: keys u64, dm f32 the measured depth there, px, py their integer coordinates
    -> terms int64 (P,30) (28 quantised terms, covered, count; zero rows where nothing is added), status bits, and the
    floating-point values of the associated pixels for the tests: {"assoc" mask, "yy", "terms" float (P,28)}."""
    keys = np.asarray(keys, np.uint64).reshape(-1)
    dm = np.asarray(dm, np.float32).reshape(-1).astype(np.float64)
    px, py = np.asarray(px, np.int64).reshape(-1).astype(np.float64), np.asarray(py, np.int64).reshape(-1).astype(np.float64)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    P = np.asarray(pose, np.float64).reshape(4, 4)
    k = np.asarray(K, np.float64).reshape(9)
    F, n = len(c), len(keys)
    out = np.zeros((n, 30), np.int64)
    status = 0
    covered = keys != raster_ref.EMPTY_KEY
    out[covered, COVERED] = 1
    f = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    zr = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    known = covered & (f < F)
    if (covered & ~known).any():
        status |= BAD_INDEX
    cf = c[np.where(known, f, 0)] if F else np.zeros((n, 3))
    with np.errstate(all="ignore"):
        r = dm - zr
        m = [(P[i, 0] * cf[:, 0] + P[i, 1] * cf[:, 1]) + P[i, 2] * cf[:, 2] for i in range(3)]
        mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        finite = mm < np.inf
        if (known & ~finite).any():
            status |= BAD_INDEX
        near = (np.abs(r) < gate) if variant == "strict_gate" else (np.abs(r) <= gate)
        assoc = known & finite & (dm > 0) & (dm < np.inf) & near & (mm > 0)
        b = (py - k[5]) / k[4]
        a = ((px - k[2]) - k[1] * b) / k[0]
        q = [a * zr, b * zr, zr]
        d = [r * a, r * b, r]
        origin = (0.0, 0.0, 0.0) if variant == "camera_origin" else P[:3, 3]
        y = [(q[i] - origin[i]) / scale for i in range(3)]
        yy = (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]
        cross = [y[1] * m[2] - y[2] * m[1], y[2] * m[0] - y[0] * m[2], y[0] * m[1] - y[1] * m[0]]
        if variant == "cross_swapped":
            cross = [m[1] * y[2] - m[2] * y[1], m[2] * y[0] - m[0] * y[2], m[0] * y[1] - m[1] * y[0]]
        g = cross + m
        e = ((m[0] * d[0] + m[1] * d[1]) + m[2] * d[2]) / scale
        w = 1.0 / mm
        if variant == "weight_inv_norm":
            w = 1.0 / np.sqrt(mm)
        h = [w * gi for gi in g]
        ee = (w * e) * e
        keep = yy <= TERM_MAX
        for i in range(6):
            keep &= (h[i] * g[i] <= TERM_MAX)
        keep &= ee <= TERM_MAX
        if (assoc & ~keep).any():
            status |= RANGE
        assoc &= keep
        terms = [h[i] * g[j] for i, j in PAIRS] + [h[i] * e for i in range(6)] + [ee]
        terms = np.stack(terms, axis=1)
        rounded = (np.floor if variant == "floor" else np.rint)(np.where(assoc[:, None], terms, 0.0) * QUANTUM)
    out[:, :28] = rounded.astype(np.int64)
    out[assoc, COUNT] = 1
    return out, status, dict(assoc=assoc, yy=yy, terms=terms)


def accumulate(vis, c, poses, K, depth, frame, box, gate, scale, variant=None):
    """vis (N,H,W) u64, c (F,3), poses (N,4,4), K (N,9), depth (M,H,W) f32, frame (N), box (N,4), gate (N), scale (N)
    -> sums (N,32) int64, status (N) int32."""
    vis = np.asarray(vis).view(np.uint64)
    N, H, W = vis.shape
    depth = np.asarray(depth, np.float32)
    sums, status = np.zeros((N, SUMS), np.int64), np.zeros(N, np.int32)
    for n in range(N):
        x0, y0, x1, y1 = clamp_box(box[n], H, W)
        if x1 < x0 or y1 < y0:
            continue
        if not 0 <= int(frame[n]) < len(depth):
            status[n] = BAD_INDEX
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        terms, status[n], _ = pixel_terms(vis[n, y0:y1 + 1, x0:x1 + 1], depth[int(frame[n]), y0:y1 + 1, x0:x1 + 1], px, py, c, poses[n], K[n],
                                          float(gate[n]), float(scale[n]), variant)
        sums[n, :30] = terms.sum(axis=0)
    return sums, status


def normal_equations(row):
    """One row of sums -> A (6,6) symmetric, rhs (6,), as floats: (double)sum * 2^-36."""
    A = np.zeros((6, 6))
    for o, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = float(int(row[o])) * 2.0 ** -36
    return A, np.asarray([float(int(row[RHS + i])) * 2.0 ** -36 for i in range(6)])


def ldl_solve(A, rhs, thr):
    """The header's unpivoted LDL^T on Python floats -> (x, pivots, index of the first pivot not above thr or None)."""
    A = [[float(v) for v in r] for r in np.asarray(A)]
    L = [[0.0] * 6 for _ in range(6)]
    D, pivots = [0.0] * 6, []
    for j in range(6):
        u = [L[j][k] * D[k] for k in range(j)]
        p = A[j][j]
        for k in range(j):
            p = p - L[j][k] * u[k]
        pivots.append(p)
        if not p > thr:
            return None, pivots, j
        D[j] = p
        for i in range(j + 1, 6):
            s = A[j][i]
            for k in range(j):
                s = s - L[i][k] * u[k]
            L[i][j] = s / p
    x = [float(v) for v in rhs]
    for i in range(6):
        for k in range(i):
            x[i] = x[i] - L[i][k] * x[k]
    for i in range(6):
        x[i] = x[i] / D[i]
    for i in range(5, -1, -1):
        for k in range(i + 1, 6):
            x[i] = x[i] - L[k][i] * x[k]
    return x, pivots, None


def cayley(omega, variant=None):
    """(3,3) float64: ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) with a = omega / 2, in the header's order."""
    h = 1.0 if variant == "full_omega" else 0.5
    a0, a1, a2 = (h * float(v) for v in omega)
    a00, a11, a22, a01, a02, a12 = a0 * a0, a1 * a1, a2 * a2, a0 * a1, a0 * a2, a1 * a2
    s = (a00 + a11) + a22
    p, q = 1.0 - s, 1.0 + s
    return np.asarray([[(p + 2.0 * a00) / q, (2.0 * a01 - 2.0 * a2) / q, (2.0 * a02 + 2.0 * a1) / q],
                       [(2.0 * a01 + 2.0 * a2) / q, (p + 2.0 * a11) / q, (2.0 * a12 - 2.0 * a0) / q],
                       [(2.0 * a02 - 2.0 * a1) / q, (2.0 * a12 + 2.0 * a0) / q, (p + 2.0 * a22) / q]])


def update(sums, clipped, scale, start, min_points, min_pivot, damping, tol2, poses, state, variant=None):
    """-> new poses (N,4,4) f64, their f32 conversions, state.  The kernel leaves the f32 copy of a pair alone where it leaves the
    pair alone (stopped before; or stopping now without `start`): the conversion returned here is that pair's only if the
    caller's copy was the conversion of its pose."""
    poses, state = np.array(poses, np.float64, copy=True), np.array(state, np.int32, copy=True)
    for n in range(len(poses)):
        st = int(state[n])
        if st & STOP:
            continue
        count = int(sums[n][COUNT])
        stop, x = 0, None
        if clipped is not None and int(clipped[n]) != 0:
            stop = CLIPPED
        elif count < min_points:
            stop = FEW
        else:
            A, rhs = normal_equations(sums[n])
            cnt = float(count)
            for i in range(6):
                A[i, i] = A[i, i] + damping * cnt
            x, _, bad = ldl_solve(A, rhs, min_pivot * cnt)
            if bad is None:
                xx = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]
            if bad is not None or not xx < np.inf:
                stop = DEGENERATE
        if stop:
            state[n] = (st & ~CONVERGED) | stop
            if start is not None:
                poses[n] = start[n]
            continue
        Q, P = cayley(x[:3], variant), poses[n].copy()
        sc = 1.0 if variant == "unscaled_t" else float(scale[n])
        for i in range(3):
            for j in range(3):
                poses[n, i, j] = (Q[i, 0] * P[0, j] + Q[i, 1] * P[1, j]) + Q[i, 2] * P[2, j]
            poses[n, i, 3] = P[i, 3] + sc * x[3 + i]
        state[n] = (st & ~CONVERGED) | (CONVERGED if xx < tol2 else 0)
    return poses, poses.astype(np.float32), state


def refine(vertices, faces, poses, K, depth, frame, box, gate, scale, iters, min_points, min_pivot, damping, tol2, H, W, znear=1e-3,
           variant=None):
    """DepthRefiner's loop on the host: iters x (project -> raster -> accumulate -> update) and one last project / raster /
    accumulate.  K (N,9) (one camera per pair; raster_ref.project takes one at a time).
    -> {"poses" (N,4,4) f64, "state", "status" (the final accumulate's), "sums" (the final accumulate's)}."""
    poses = np.array(poses, np.float64, copy=True)
    N = len(poses)
    start, K = poses.copy(), np.asarray(K, np.float64).reshape(N, 9)
    c = face_normals(vertices, faces)
    state, p32 = np.zeros(N, np.int32), poses.astype(np.float32)

    def draw():
        vis, clipped = np.zeros((N, H, W), np.uint64), np.zeros(N, np.int32)
        for n in range(N):
            xy, vd = raster_ref.project(vertices, p32[n:n + 1], K[n], znear)
            vis[n:n + 1], clipped[n:n + 1] = raster_ref.raster(xy, vd, faces, H, W)
        return vis, clipped

    for _ in range(iters):
        vis, clipped = draw()
        sums, _ = accumulate(vis, c, poses, K, depth, frame, box, gate, scale, variant)
        poses, p32, state = update(sums, clipped, scale, start, min_points, min_pivot, damping, tol2, poses, state, variant)
    vis, clipped = draw()
    sums, status = accumulate(vis, c, poses, K, depth, frame, box, gate, scale, variant)
    late = (clipped != 0) & ((state & STOP) == 0)           # the LAST view is the first that drops a triangle: the input pose
    poses[late], state[late] = start[late], state[late] | CLIPPED
    return dict(poses=poses, state=state, status=status, sums=sums, clipped=clipped)
