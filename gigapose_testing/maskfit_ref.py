"""libgigapose_maskfit.so restated in numpy / Python from the description in include/gigapose_maskfit.h (the arithmetic there is
the contract): the moments of a run-length mask in closed form, the moments of a drawing's covered pixels with its intersection
with the mask and its box-edge count, and the rational update of the four degrees of freedom a silhouette holds.  The GPU tests
compare the kernels with this bit for bit; the loop at the end (refine) is MaskRefiner.refine over raster_ref's rasteriser.

`variant` selects a deliberately WRONG fitter (tests/test_maskfit_host.py shows that its checks reject each): None is the
contract."""
import numpy as np

from . import raster_ref, verify_ref

ROW, MM = 16, 8
N_, SX, SY, SXX, SXY, SYY, INTER, EDGE = range(8)
BAD_MASK, NO_MASK, FEW, CLIPPED, ROUND, NOT_IMPROVED = 1, 2, 4, 8, 16, 32
STOP = BAD_MASK | NO_MASK | FEW | CLIPPED
VARIANTS = ("row_major", "run_end", "turn_sign", "g_inverted", "shift_without_g", "keep_last", "float_ties")


def clamp_box(box, H, W):
    x0, y0, x1, y1 = (int(b) for b in box)
    return max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)


def _s1(m):
    return m * (m + 1) // 2                      # 0 + 1 + .. + m;  0 for m = -1


def _s2(m):
    return m * (m + 1) * (2 * m + 1) // 6        # 0 + 1 + 4 + .. + m*m;  0 for m = -1


def segment(x, ya, yb):
    """The six sums of the pixels (x, ya .. yb) of one column, Python integers."""
    cnt = yb - ya + 1
    sy, syy = _s1(yb) - _s1(ya - 1), _s2(yb) - _s2(ya - 1)
    return [cnt, x * cnt, sy, x * x * cnt, x * sy, syy]


def columns(xa, xb, H):
    """The six sums of the full columns xa .. xb."""
    nc = xb - xa + 1
    sx, sxx = _s1(xb) - _s1(xa - 1), _s2(xb) - _s2(xa - 1)
    return [nc * H, H * sx, nc * _s1(H - 1), H * sxx, sx * _s1(H - 1), nc * _s2(H - 1)]


def run_sums(a, b, H):
    """The run of ones over the pixel indices [a, b), p = x*H + y, 0 <= a < b: head segment, full columns, tail segment."""
    xa, ya, xb, yb = a // H, a % H, (b - 1) // H, (b - 1) % H
    if xa == xb:
        return segment(xa, ya, yb)
    parts = [segment(xa, ya, H - 1), segment(xb, 0, yb)]
    if xb - xa >= 2:
        parts.append(columns(xa + 1, xb - 1, H))
    return [sum(p[i] for p in parts) for i in range(6)]


def mask_moments(cum, offsets, H, W, variant=None):
    """cum int32[total], offsets int32[D+1] -> mm (D,8) int64, mstatus (D) int32."""
    cum, offsets = np.asarray(cum, np.int64).reshape(-1), np.asarray(offsets, np.int64).reshape(-1)
    D, total = len(offsets) - 1, len(cum)
    mm, mstatus = np.zeros((D, MM), np.int64), np.zeros(D, np.int32)
    for d in range(D):
        lo, hi = int(offsets[d]), int(offsets[d + 1])
        if not (0 <= lo < hi <= total) or int(cum[hi - 1]) != H * W:
            mstatus[d] = BAD_MASK
            continue
        acc = [0] * 6
        for i in range(lo + 1, hi, 2):
            a, b = int(cum[i - 1]), int(cum[i])
            if variant == "run_end":
                b += 1
            if not (0 <= a < b <= H * W):
                continue
            if variant == "row_major":               # the run read over a mask flattened row by row
                s = run_sums(a, b, W)
                s = [s[0], s[2], s[1], s[5], s[4], s[3]]
            else:
                s = run_sums(a, b, H)
            acc = [u + v for u, v in zip(acc, s)]
        mm[d, :6] = acc
    return mm, mstatus


def moments(vis, cum, offsets, det, box, variant=None):
    """vis (N,H,W) u64, cum int32[total], offsets int32[D+1], det (N), box (N,4) -> rows (N,16) int64, status (N) int32."""
    vis = np.asarray(vis).view(np.uint64)
    N, H, W = vis.shape
    cum, offsets = np.asarray(cum, np.int64).reshape(-1), np.asarray(offsets, np.int64).reshape(-1)
    total, D = len(cum), len(offsets) - 1
    rows, status = np.zeros((N, ROW), np.int64), np.zeros(N, np.int32)
    for n in range(N):
        d = int(det[n])
        if d < 0:
            status[n] = NO_MASK
            continue
        if d >= D:
            status[n] = BAD_MASK
            continue
        lo, hi = int(offsets[d]), int(offsets[d + 1])
        if not (0 <= lo < hi <= total) or int(cum[hi - 1]) != H * W:
            status[n] = BAD_MASK
            continue
        x0, y0, x1, y1 = clamp_box(box[n], H, W)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        covered = vis[n, y0:y1 + 1, x0:x1 + 1] != raster_ref.EMPTY_KEY
        inside = verify_ref.mask_bits(cum[lo:hi], px, py, H, W, "row_major" if variant == "row_major" else None) == 1
        edge = ((px == x0) & (x0 > 0)) | ((px == x1) & (x1 < W - 1)) | ((py == y0) & (y0 > 0)) | ((py == y1) & (y1 < H - 1))
        x, y = px[covered], py[covered]
        rows[n, :8] = (len(x), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), (covered & inside).sum(), (covered & edge).sum())
    return rows, status


def shape_values(s):
    """n, Sx, Sy, Sxx, Sxy, Syy (integers, n > 0) -> mx, my, a, b, tr as Python floats, in the header's order."""
    n = float(int(s[0]))
    mx, my = float(int(s[1])) / n, float(int(s[2])) / n
    uxx = float(int(s[3])) / n - mx * mx
    uxy = float(int(s[4])) / n - mx * my
    uyy = float(int(s[5])) / n - my * my
    return mx, my, uxx - uyy, 2.0 * uxy, uxx + uyy


def turn_of(D, M, e, gain, variant=None):
    """The shape values of the drawing and of the mask -> (tau, turned?)."""
    _, _, aD, bD, trD = D
    _, _, aM, bM, trM = M
    e2 = e * e
    dot = aD * aM + bD * bM
    cross = aD * bM - bD * aM
    ok = (aD * aD + bD * bD >= e2 * (trD * trD)) and (aM * aM + bM * bM >= e2 * (trM * trM)) and dot > 0.0 and abs(cross) <= dot
    if not ok:
        return 0.0, False
    tau = (gain * (cross / dot)) / 4.0
    return (-tau if variant == "turn_sign" else tau), True


def step(row, m, K, P, e, gain, variant=None):
    """One pair's next pose: row (16) and m (8) integers, K 9 floats, P (4,4) -> (new pose (4,4), turned?)."""
    k = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    D, M = shape_values(row), shape_values(m)
    tau, turned = turn_of(D, M, e, gain, variant)
    tt = tau * tau
    den = 1.0 + tt
    c, s = (1.0 - tt) / den, (2.0 * tau) / den
    P = np.array(P, np.float64, copy=True)
    Q = P.copy()
    for j in range(4):
        Q[0, j] = c * P[0, j] - s * P[1, j]
        Q[1, j] = s * P[0, j] + c * P[1, j]
    g = (1.0 + float(int(row[0])) / float(int(m[0]))) / 2.0
    if variant == "g_inverted":
        g = (1.0 + float(int(m[0])) / float(int(row[0]))) / 2.0
    g = 1.0 + gain * (g - 1.0)
    g = 0.5 if g < 0.5 else (2.0 if g > 2.0 else g)
    t0, t1, t2 = float(Q[0, 3]), float(Q[1, 3]), float(Q[2, 3])
    ox = ((k[0] * t0 + k[1] * t1) + k[2] * t2) / t2
    oy = ((k[3] * t0 + k[4] * t1) + k[5] * t2) / t2
    dx, dy = D[0] - k[2], D[1] - k[5]
    px, py = k[2] + (c * dx - s * dy), k[5] + (s * dx + c * dy)
    if variant == "shift_without_g":
        qx, qy = px, py
    else:
        qx, qy = ox + (px - ox) / g, oy + (py - oy) / g
    t0, t1, t2 = g * t0, g * t1, g * t2
    Q[0, 3] = t0 + ((gain * (M[0] - qx)) * t2) / k[0]
    Q[1, 3] = t1 + ((gain * (M[1] - qy)) * t2) / k[4]
    Q[2, 3] = t2
    return Q, turned


def new_state(N):
    return dict(best=np.zeros((N, 4, 4)), score=np.zeros((N, 4), np.int64), state=np.zeros((N, 2), np.int32))


def update(rows, status, mm, det, clipped, K, start, it, last, min_points, e, gain, poses, st, variant=None):
    """-> new poses (N,4,4) f64, their f32 conversions, the new state {"best" (N,4,4), "score" (N,4) inter, union of the best and
    of the start, "state" (N,2) bits, best iteration}.  The f32 copy returned is the kernel's only where the kernel writes it (a
    pair that is stopped already is not touched)."""
    poses = np.array(poses, np.float64, copy=True)
    best, score, state = (np.array(st[k], copy=True) for k in ("best", "score", "state"))
    D = len(mm)
    for n in range(len(poses)):
        if it == 0:
            best[n], score[n], state[n] = poses[n], (0, 1, 0, 1), (0, 0)
        bits = int(state[n, 0])
        if bits & STOP:
            continue
        d = int(det[n])
        stop = int(status[n]) & (BAD_MASK | NO_MASK)
        if not stop and not 0 <= d < D:
            stop = NO_MASK if d < 0 else BAD_MASK
        if clipped is not None and int(clipped[n]) != 0:
            stop |= CLIPPED
        r = [int(v) for v in rows[n]]
        m = [int(v) for v in mm[d]] if not stop else None
        if not stop and (r[N_] < min_points or m[N_] < min_points):
            stop = FEW
        if stop:
            state[n] = (bits & ~ROUND) | stop | NOT_IMPROVED, 0
            poses[n] = best[n] = start[n]
            score[n, :2] = score[n, 2:]
            continue
        inter, union = r[INTER], r[N_] + m[N_] - r[INTER]
        if it == 0:
            score[n] = (inter, union, inter, union)
        else:
            ib, ub = int(score[n, 0]), int(score[n, 1])
            better = inter * ub > ib * union
            if variant == "float_ties":
                better = inter / union >= ib / ub
            if variant == "keep_last":
                better = True
            if r[EDGE] == 0 and better:
                best[n], score[n, :2], state[n, 1] = poses[n], (inter, union), it
        if last:
            poses[n] = best[n]
            if state[n, 1] == 0:
                state[n, 0] = bits | NOT_IMPROVED
            continue
        poses[n], turned = step(r, m, K[n], poses[n], e, gain, variant)
        state[n, 0] = (bits & ~ROUND) | (0 if turned else ROUND)
    return poses, poses.astype(np.float32), dict(best=best, score=score, state=state)


def cum_of(lists):
    """Run-length lists -> (cum int32, offsets int32): what gpi_rle_scan leaves."""
    lists = [np.asarray(m, np.int64) for m in lists]
    cum = np.concatenate([np.cumsum(m) for m in lists]) if lists else np.zeros(0, np.int64)
    return cum.astype(np.int32), np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int32)


def refine(vertices, faces, poses, K, lists, det, box, iters, min_points, e, gain, H, W, znear=1e-3, variant=None):
    """MaskRefiner's loop on the host: iters x (project -> raster -> moments -> update), then one last draw, moments and an update
    that only judges.  K (N,9); lists: one run-length list per detection; det (N) into them.
    -> {"poses" (N,4,4) f64: the best, "state" (N,2), "score" (N,4), "rows": the last moments}."""
    poses = np.array(poses, np.float64, copy=True)
    N = len(poses)
    start, K = poses.copy(), np.asarray(K, np.float64).reshape(N, 9)
    cum, offsets = cum_of(lists)
    mm, _ = mask_moments(cum, offsets, H, W, variant)
    st, p32 = new_state(N), poses.astype(np.float32)
    for it in range(iters + 1):
        vis, clipped = np.zeros((N, H, W), np.uint64), np.zeros(N, np.int32)
        for n in range(N):
            xy, vd = raster_ref.project(vertices, p32[n:n + 1], K[n], znear)
            vis[n:n + 1], clipped[n:n + 1] = raster_ref.raster(xy, vd, faces, H, W)
        rows, status = moments(vis, cum, offsets, det, box, variant)
        poses, p32, st = update(rows, status, mm, det, clipped, K, start, it, it == iters, min_points, e, gain, poses, st, variant)
    return dict(poses=poses, state=st["state"], score=st["score"], rows=rows, mm=mm)
