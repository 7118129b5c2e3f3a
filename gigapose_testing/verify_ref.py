"""libgigapose_verify.so restated in numpy from the description in include/gigapose_verify.h (the arithmetic there is the
contract): the class of every pixel of a hypothesis's box against the sensor's depth, its bit of the detection's run-length
mask, the sixteen counts.  The GPU tests compare the kernel with this bit for bit; score_drawn / select at the end are
HypothesisVerifier's host half over raster_ref's rasteriser, written from the issue's formulae and sharing nothing with
gigapose_amd/verify.py but the constants.

`variant` selects a deliberately WRONG verifier (tests/test_verify_host.py shows that its checks reject each): None is the
contract."""
import numpy as np

from . import raster_ref

COUNTS = 16
UNMEASURED, AGREE, BEHIND, FRONT = 0, 1, 2, 3
UNCOVERED_IN_MASK, RESIDUAL = 8, 9
QUANTUM = 2.0 ** 20
BAD_FRAME, BAD_MASK = 1, 2
VARIANTS = ("swapped", "row_major", "strict_gate", "iou_covered_only", "late_ties", "strict_rank")


def clamp_box(box, H, W):
    x0, y0, x1, y1 = (int(b) for b in box)
    return max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)


def mask_bits(cum, px, py, H, W, variant=None):
    """The prefix sums of ONE detection's run lengths, pixels px, py -> the mask bit of each: the parity of #{i : cum[i] <= p},
    p = px*H + py."""
    cum = np.asarray(cum, np.int64).reshape(-1)
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    p = py * W + px if variant == "row_major" else px * H + py
    below = (cum[None, :] < p.reshape(-1, 1)) if variant == "strict_rank" else (cum[None, :] <= p.reshape(-1, 1))
    return (below.sum(axis=1) & 1).reshape(p.shape)


def pixel_classes(keys, dm, tol, variant=None):
    """keys u64 and dm f32 (or None: no depth image) of any one shape, tol a float -> covered (bool), class (int, of the covered
    pixels; 0 elsewhere), the quantised residual (int64, 0 unless the class is AGREE)."""
    keys = np.asarray(keys, np.uint64)
    covered = keys != raster_ref.EMPTY_KEY
    cls, res = np.zeros(keys.shape, np.int64), np.zeros(keys.shape, np.int64)
    if dm is None:
        return covered, cls, res
    zr = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    dm = np.asarray(dm, np.float32).astype(np.float64)
    t = np.float64(tol)
    with np.errstate(all="ignore"):
        measured = covered & (dm > 0) & (dm < np.inf)
        r = dm - zr
        near = (np.abs(r) < t) if variant == "strict_gate" else (np.abs(r) <= t)
        behind, front = ~near & (r > t), ~near & ~(r > t) & (r < -t)
        if variant == "swapped":
            behind, front = front, behind
        cls[measured & near] = AGREE
        cls[measured & behind] = BEHIND
        cls[measured & front] = FRONT
        q = np.abs(r) / t if t > 0 else np.zeros_like(r)
        q = np.where(measured & near & ~np.isnan(q), q, 0.0)
        res = np.rint(q * QUANTUM).astype(np.int64)
    return covered, cls, res


def counts(vis, depth, frame, cum, offsets, det, box, tol, variant=None):
    """vis (N,H,W) u64, depth (M,H,W) f32 or None, frame (N), cum int32[total] + offsets int32[D+1] or None, det (N) (ignored
    without cum), box (N,4), tol (N) -> counts (N,16) int64, status (N) int32."""
    vis = np.asarray(vis).view(np.uint64)
    N, H, W = vis.shape
    out, status = np.zeros((N, COUNTS), np.int64), np.zeros(N, np.int32)
    if depth is not None:
        depth = np.asarray(depth, np.float32)
    if cum is not None:
        cum, offsets = np.asarray(cum, np.int64), np.asarray(offsets, np.int64)
        total, D = len(cum), len(offsets) - 1
    for n in range(N):
        bad, lists = 0, None
        if depth is not None and not 0 <= int(frame[n]) < len(depth):
            bad |= BAD_FRAME
        if cum is not None and int(det[n]) >= 0:
            d = int(det[n])
            if d >= D:
                bad |= BAD_MASK
            else:
                lo, hi = int(offsets[d]), int(offsets[d + 1])
                if not (0 <= lo < hi <= total) or int(cum[hi - 1]) != H * W:
                    bad |= BAD_MASK
                else:
                    lists = cum[lo:hi]
        if bad:
            status[n] = bad
            continue
        x0, y0, x1, y1 = clamp_box(box[n], H, W)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        keys = vis[n, y0:y1 + 1, x0:x1 + 1]
        dm = None if depth is None else depth[int(frame[n]), y0:y1 + 1, x0:x1 + 1]
        covered, cls, res = pixel_classes(keys, dm, float(tol[n]), variant)
        inside = np.zeros(keys.shape, np.int64) if lists is None else mask_bits(lists, px, py, H, W, variant)
        slot = np.where(covered, 2 * cls + inside, np.where(inside == 1, UNCOVERED_IN_MASK, -1))
        for s in range(9):
            out[n, s] = int((slot == s).sum())
        out[n, RESIDUAL] = int(res[covered].sum())
    return out, status


# ------------------------------------------------------------------------------------------------ the scores (host, float64)
def scores(c, mask_area=None, status=None, clipped=None, min_points=32, occlusion_weight=0.0, tol=None, has_depth=True, variant=None):
    """Rows of counts -> {"verify", "depth_fit", "iou", "residual"} as float64 arrays, by the issue's formulae, one pair at a
    time in Python floats.  mask_area (N): the area of each pair's mask over the whole frame, NaN or None = the pair has no mask."""
    c = np.asarray(c, np.int64).reshape(-1, COUNTS)
    N = len(c)
    out = {k: np.zeros(N) for k in ("verify", "depth_fit", "iou", "residual")}
    for n in range(N):
        r = [int(v) for v in c[n]]
        area = None if mask_area is None or np.isnan(float(mask_area[n])) else float(mask_area[n])
        agree, behind = r[2] + r[3], r[4] + r[5]
        covered = sum(r[:8])
        inter = r[1] + r[3] + r[5] + r[7]
        front = float(r[6] + r[7]) if area is None else r[7] + float(occlusion_weight) * r[6]
        fit = 0.0 if agree < min_points or agree + behind + front == 0 else agree / (agree + behind + front)
        iou = 0.0
        if area is not None:
            union = covered + area - inter
            if variant == "iou_covered_only":
                union = float(covered)
            iou = inter / union if union != 0 else 0.0
        if has_depth and area is not None:
            v = fit * iou
        elif has_depth:
            v = fit
        else:
            v = iou
        if covered == 0 or (status is not None and int(status[n]) != 0) or (clipped is not None and int(clipped[n]) != 0):
            v = 0.0
        t = np.nan if tol is None else float(np.asarray(tol, np.float64).reshape(-1)[n if np.size(tol) > 1 else 0])
        out["verify"][n], out["depth_fit"][n], out["iou"][n] = v, fit, iou
        out["residual"][n] = t * r[RESIDUAL] * 2.0 ** -20 / agree if agree else np.nan
    return out


def mask_area_of(counts_list):
    """One detection's run lengths -> the number of set pixels: the sum of the odd-numbered counts."""
    return int(np.asarray(counts_list, np.int64)[1::2].sum())


def draw_poses(vertices, faces, poses, K, H, W, znear=1e-3):
    """poses (N,4,4) f64, drawn from their f32 conversions by raster_ref -> keys (N,H,W) u64, clipped (N) int32."""
    poses = np.asarray(poses, np.float64)
    N = len(poses)
    vis, clipped = np.zeros((N, H, W), np.uint64), np.zeros(N, np.int32)
    for n in range(N):
        xy, vd = raster_ref.project(vertices, poses[n:n + 1].astype(np.float32), np.asarray(K, np.float64).reshape(9), znear)
        vis[n:n + 1], clipped[n:n + 1] = raster_ref.raster(xy, vd, faces, H, W)
    return vis, clipped


def score_drawn(drawn, depth, frame, masks, det, box, tol, min_points=32, occlusion_weight=0.0, variant=None):
    """HypothesisVerifier.score's arithmetic on the host: drawn = (keys, clipped) from draw_poses, depth (M,H,W) or None, masks =
    list of run-length lists (one per detection) or None, det (N) into it (-1: none)
    -> (counts (N,16), status (N), the dict of scores)."""
    vis, clipped = drawn
    cum = offsets = area = None
    if masks is not None:
        lists = [np.asarray(m, np.int64) for m in masks]
        cum = np.concatenate([np.cumsum(m) for m in lists]) if lists else np.zeros(0, np.int64)
        offsets = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)
        area = np.asarray([mask_area_of(lists[int(d)]) if int(d) >= 0 else np.nan for d in det], np.float64)
    c, status = counts(vis, depth, frame, cum, offsets, det, box, tol, variant)
    return c, status, scores(c, area, status, clipped, min_points, occlusion_weight, tol, depth is not None, variant)


def select(verify, coarse, instance, variant=None):
    """verify, coarse (E,) floats, instance (E,) hashable keys -> the index kept per instance, in the order of first appearance:
    the largest verify, a tie to the larger coarse score, then to the earlier position."""
    order, best = [], {}
    for i, key in enumerate(instance):
        if key not in best:
            order.append(key)
            best[key] = i
            continue
        j = best[key]
        a, b = (float(verify[i]), float(coarse[i])), (float(verify[j]), float(coarse[j]))
        if a > b or (variant == "late_ties" and a == b):
            best[key] = i
    return [best[k] for k in order]
