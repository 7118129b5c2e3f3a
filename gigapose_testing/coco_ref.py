"""include/gigapose_coco.h and the host half of gigapose_amd/detections.py restated in numpy and Python integers: what
libgigapose_coco.so is held to BIT FOR BIT (tests/test_gpu_coco.py), itself held to independent readings -- dense masks and pixel
sets, fractions.Fraction IoUs, Fraction precisions -- by tests/test_coco_host.py.  Written from the header and COCO's definition,
not from the kernels.

  fg_scan(cum, offsets, HW, fg)                       -> fg, area, status
  mask_inter(A, B, HW, pair_a, pair_b)                A, B = (cum, offsets, fg)  -> inter, status
  box_inter(boxA, boxB, pair_a, pair_b)               -> inter, area_a, area_b, status
  match(det_off, gt_off, pair_off, inter, area_det, area_gt, gt_ignore, thr_num, thr_den)   -> dt_match, dt_ignore, status
  sup_bits(inter, area, num, den)                     -> sup u64 (P, words);  mask_nms: + the greedy pass of label_ref
  average_precision(groups, thresholds, thr_den)      the AP arithmetic of detections.average_precision
  evaluate(images, ...)                               a whole DetectionScorer.score on host lists
VARIANTS are subtly wrong versions; tests/test_coco_host.py shows that its checks reject each of them, and tests/test_gpu_coco.py
names the GPU test that would fail with each of them standing in for the kernels.
"""
import math

import numpy as np

from . import label_ref

BAD_MASK = 1
PAIR_RANGE, PAIR_MASK = 1, 2
GROUP_RANGE, GROUP_ORDER, GROUP_SIZE = 1, 2, 4
MAX_GROUP_GT, MAX_COORD = 4096, 1 << 21
VARIANTS = ("even_runs", "search_one_short", "strict_threshold", "first_on_tie", "no_ignore_preference", "rematch", "no_envelope",
            "float_recall")
# A search that is off by one only AT x == cum[j] (the first j with cum[j] >= x) is NOT wrong: F_M is continuous at the end of a
# run -- the run that ends at x contributes all of its pixels either way -- so both searches give the same numbers.
HARMLESS = ("search_off_by_one",)


# ------------------------------------------------------------------------------------------------ masks
def mask_slice(cum, offsets, d, HW):
    """-> (lo, hi) of mask d, or None when it is BAD."""
    lo, hi = int(offsets[d]), int(offsets[d + 1])
    if not (0 <= lo < hi <= len(cum)) or int(cum[hi - 1]) != HW:
        return None
    return lo, hi


def fg_scan(cum, offsets, HW, fg=None, variant=None):
    """fg: the buffer's contents before the call (a BAD mask's part is not written); default zeros."""
    cum = np.asarray(cum, np.int32)
    D = len(offsets) - 1
    fg = np.zeros(len(cum), np.int32) if fg is None else np.array(fg, np.int32)
    area, status = np.zeros(D, np.int64), np.zeros(D, np.int32)
    for d in range(D):
        s = mask_slice(cum, offsets, d, HW)
        if s is None:
            status[d] = BAD_MASK
            continue
        lo, hi = s
        lens = np.diff(cum[lo:hi].astype(np.int64), prepend=0)
        lens[(1 if variant == "even_runs" else 0)::2] = 0              # run i is foreground iff i is odd
        sums = np.cumsum(lens)
        fg[lo:hi] = sums.astype(np.int32)                              # truncated to 32 bits
        area[d] = sums[-1]
    return fg, area, status


def fg_below(c, f, x, variant=None):
    """F_M(x) of the header for a mask's slices c = cum[lo:hi], f = fg[lo:hi] (int64) and an int64 array x.  numpy.searchsorted is
    the binary search for a non-decreasing c, which is what a scan writes."""
    n = len(c)
    j = np.searchsorted(c, x, side="left" if variant == "search_off_by_one" else "right")      # the first j with c[j] > x
    if variant == "search_one_short":
        j = np.maximum(j - 1, 0)                                       # the last j with c[j] <= x
    below = np.where(j > 0, f[np.maximum(j, 1) - 1], 0)
    inside = (j < n) & (j % 2 == 1)
    return below + np.where(inside, x - c[np.maximum(j, 1) - 1], 0)


def mask_inter(A, B, HW, pair_a, pair_b, variant=None):
    (cumA, offA, fgA), (cumB, offB, fgB) = A, B
    P = len(pair_a)
    inter, status = np.zeros(P, np.int64), np.zeros(P, np.int32)
    for p in range(P):
        a, b = int(pair_a[p]), int(pair_b[p])
        if not (0 <= a < len(offA) - 1 and 0 <= b < len(offB) - 1):
            status[p] = PAIR_RANGE
            continue
        sa, sb = mask_slice(cumA, offA, a, HW), mask_slice(cumB, offB, b, HW)
        if sa is None or sb is None:
            status[p] = PAIR_MASK
            continue
        walk_a = sa[1] - sa[0] <= sb[1] - sb[0]                        # the mask with fewer runs is walked, A's on a tie
        (wc, ws), (sc, sf, ss) = ((cumA, sa), (cumB, fgB, sb)) if walk_a else ((cumB, sb), (cumA, fgA, sa))
        w = np.asarray(wc[ws[0]:ws[1]], np.int64)
        c, f = np.asarray(sc[ss[0]:ss[1]], np.int64), np.asarray(sf[ss[0]:ss[1]], np.int64)
        inter[p] = int((fg_below(c, f, w[1::2], variant) - fg_below(c, f, w[0:len(w) - 1:2], variant)).sum())     # ends - starts of the odd runs
    return inter, status


def _clamp(v):
    return min(max(int(v), -MAX_COORD), MAX_COORD)


def _area(x0, y0, x1, y1):
    return max(0, x1 - x0) * max(0, y1 - y0)


def box_inter(boxA, boxB, pair_a, pair_b):
    P = len(pair_a)
    out = np.zeros((3, P), np.int64)
    status = np.zeros(P, np.int32)
    for p in range(P):
        a, b = int(pair_a[p]), int(pair_b[p])
        if not (0 <= a < len(boxA) and 0 <= b < len(boxB)):
            status[p] = PAIR_RANGE
            continue
        A, B = [_clamp(v) for v in boxA[a]], [_clamp(v) for v in boxB[b]]
        out[:, p] = _area(max(A[0], B[0]), max(A[1], B[1]), min(A[2], B[2]), min(A[3], B[3])), _area(*A), _area(*B)
    return out[0], out[1], out[2], status


# ------------------------------------------------------------------------------------------------ matching
def match_group(inter, area_det, area_gt, ignore, num, den, variant=None):
    """One group at one threshold: inter a D x G list of lists of Python integers -> (matches, ignore flags), D entries each."""
    D, G = len(area_det), len(area_gt)
    taken, matches, flags = set(), [], []
    for d in range(D):
        best = None                                                    # (ignored, inter, union, g)
        for g in range(G):
            if g in taken and variant != "rematch":
                continue
            i = inter[d][g]
            u = area_det[d] + area_gt[g] - i
            if u <= 0 or (i * den <= num * u if variant == "strict_threshold" else i * den < num * u):
                continue
            c = (0 if variant == "no_ignore_preference" else int(ignore[g] != 0), i, u, g)
            if best is None:
                best = c
            elif c[0] != best[0]:
                best = c if c[0] < best[0] else best
            elif c[1] * best[2] > best[1] * c[2] or (c[1] * best[2] == best[1] * c[2] and variant != "first_on_tie"):
                best = c                                               # g ascends: on equal IoUs the LAST one stands
        matches.append(-1 if best is None else best[3])
        flags.append(0 if best is None else int(ignore[best[3]] != 0))
        if best is not None:
            taken.add(best[3])
    return matches, flags


def match(det_off, gt_off, pair_off, inter, area_det, area_gt, gt_ignore, thr_num, thr_den, variant=None, dt_match=None, dt_ignore=None):
    """dt_match, dt_ignore: the buffers' contents before the call (a group with GROUP_RANGE writes nothing); default -1 and 0."""
    Q, T, TD = len(pair_off), len(thr_num), len(area_det)
    dt_match = np.full((T, TD), -1, np.int32) if dt_match is None else np.array(dt_match, np.int32)
    dt_ignore = np.zeros((T, TD), np.uint8) if dt_ignore is None else np.array(dt_ignore, np.uint8)
    status = np.zeros(Q, np.int32)
    inter_l, ad, ag, ig = np.asarray(inter).tolist(), np.asarray(area_det).tolist(), np.asarray(area_gt).tolist(), np.asarray(gt_ignore).tolist()
    for q in range(Q):
        d0, d1, g0, g1, po = int(det_off[q]), int(det_off[q + 1]), int(gt_off[q]), int(gt_off[q + 1]), int(pair_off[q])
        D, G = d1 - d0, g1 - g0
        if not (0 <= d0 <= d1 <= TD and 0 <= g0 <= g1 <= len(ag) and po >= 0 and po + D * G <= len(inter_l)):
            status[q] = GROUP_RANGE
            continue
        if G > MAX_GROUP_GT:
            status[q] = GROUP_SIZE
        elif any(ig[g0 + g - 1] != 0 and ig[g0 + g] == 0 for g in range(1, G)):
            status[q] = GROUP_ORDER
        if status[q]:
            dt_match[:, d0:d1], dt_ignore[:, d0:d1] = -1, 0
            continue
        block = [inter_l[po + d * G:po + (d + 1) * G] for d in range(D)]
        for t in range(T):
            m, f = match_group(block, ad[d0:d1], ag[g0:g1], ig[g0:g1], int(thr_num[t]), int(thr_den), variant)
            dt_match[t, d0:d1], dt_ignore[t, d0:d1] = m, f
    return dt_match, dt_ignore, status


# ------------------------------------------------------------------------------------------------ NMS on mask IoUs
def sup_bits(inter, area, num, den):
    """numpy int64 throughout: |inter|, |area| < 2^44 and den <= 2^16 keep the products below 2^62."""
    P = len(area)
    words = (P + 63) // 64
    inter, area = np.asarray(inter, np.int64).reshape(P, P), np.asarray(area, np.int64)
    union = area[:, None] + area[None, :] - inter
    hit = (inter * den > num * union) & (np.arange(P)[None, :] > np.arange(P)[:, None])
    padded = np.zeros((P, words * 64), np.uint8)
    padded[:, :P] = hit
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(P, words)


def all_pairs(P):
    """The pairs i < j in row-major order -> (pair_a, pair_b) int32."""
    i, j = np.triu_indices(P, 1)
    return i.astype(np.int32), j.astype(np.int32)


def mask_nms(cum, offsets, HW, order, num, den, variant=None):
    """Masks taken in `order` (best first) -> keep u8 (len(order),): mask j goes when a KEPT earlier mask has IoU > num / den."""
    order = np.asarray(order, np.int64)
    P = len(order)
    fg, area, status = fg_scan(cum, offsets, HW, variant=variant)
    assert not status.any()
    a, b = all_pairs(P)
    part, _ = mask_inter((cum, offsets, fg), (cum, offsets, fg), HW, order[a], order[b], variant)
    inter = np.zeros((P, P), np.int64)
    inter[a, b] = part
    return label_ref.nms_keep(sup_bits(inter, area[order], num, den), P)


# ------------------------------------------------------------------------------------------------ AP
def average_precision(groups, thresholds, thr_den, variant=None):
    """groups: per (image, category) IN IMAGE ORDER a dict(category, scores (D,) floats best first, dt_match (T, D), dt_ignore
    (T, D), npig: the number of non-ignored ground truths), each image already cut to its max_dets.  thresholds: the T numerators
    over thr_den.  -> dict(AP, AP50, AP75, AR, per_category {category: dict(AP, AP50, AP75, AR)}, cells {(category, t): (ap,
    recall, the 101 precisions)}).  A mean over no cells is -1.0.  Python integers up to the one division per precision."""
    T = len(thresholds)
    cells = {}
    for c in sorted({g["category"] for g in groups}):
        mine = [g for g in groups if g["category"] == c]
        npig = sum(int(g["npig"]) for g in mine)
        if npig == 0:
            continue
        scores = [float(s) for g in mine for s in g["scores"]]
        order = sorted(range(len(scores)), key=lambda n: -scores[n])           # sorted() is stable
        for t in range(T):
            matched = [int(m) >= 0 for g in mine for m in np.asarray(g["dt_match"]).reshape(T, -1)[t]]
            ignored = [int(i) != 0 for g in mine for i in np.asarray(g["dt_ignore"]).reshape(T, -1)[t]]
            tp, fp, ranks = 0, 0, []
            for n in order:
                if ignored[n]:
                    continue
                tp, fp = tp + matched[n], fp + (not matched[n])
                ranks.append((tp, fp))
            best = list(ranks)                                                 # non-increasing from the right, on integers
            if variant != "no_envelope":
                for r in range(len(best) - 2, -1, -1):
                    (a, b), (e, f) = best[r], best[r + 1]
                    if e * (a + b) > a * (e + f):
                        best[r] = (e, f)
            prec = []
            for i in range(101):
                if variant == "float_recall":
                    r = next((r for r, (a, _) in enumerate(ranks) if a / npig >= i * 0.01), None)
                else:
                    r = next((r for r, (a, _) in enumerate(ranks) if 100 * a >= i * npig), None)
                prec.append(0.0 if r is None else best[r][0] / (best[r][0] + best[r][1]))
            cells[(c, t)] = (math.fsum(prec) / 101, (ranks[-1][0] / npig) if ranks else 0.0, prec)
    return summarise(cells, thresholds, thr_den)


def _mean(values):
    values = list(values)
    return math.fsum(values) / len(values) if values else -1.0


def summarise(cells, thresholds, thr_den):
    def table(keys):
        at = {name: [t for t, n in enumerate(thresholds) if n * q == p * thr_den] for name, (p, q) in (("AP50", (1, 2)), ("AP75", (3, 4)))}
        return dict(AP=_mean(cells[k][0] for k in keys), AR=_mean(cells[k][1] for k in keys),
                    **{name: _mean(cells[k][0] for k in keys if k[1] in ts) for name, ts in at.items()})

    keys = sorted(cells)
    out = table(keys)
    out["per_category"] = {c: table([k for k in keys if k[0] == c]) for c in sorted({k[0] for k in keys})}
    out["cells"] = cells
    return out


# ------------------------------------------------------------------------------------------------ a whole score
def evaluate(images, thresholds=tuple(range(10, 20)), thr_den=20, max_dets=100, HW=None, variant=None):
    """images: [(gts, dets)] in image order; a gt is dict(category, ignore, cum=the mask's prefix sums | box=xyxy exclusive), a det
    dict(category, score, cum | box).  What DetectionScorer.score computes, on host lists."""
    groups = []
    for gts, dets in images:
        for c in sorted({int(x["category"]) for x in gts} | {int(x["category"]) for x in dets}):
            dt = [x for x in dets if int(x["category"]) == c]
            dt = sorted(dt, key=lambda x: -float(x["score"]))[:max_dets]
            gt = sorted((x for x in gts if int(x["category"]) == c), key=lambda x: bool(x["ignore"]))
            if dets and "cum" in dets[0] or gts and "cum" in gts[0]:
                lists = [np.asarray(x["cum"], np.int32) for x in dt + gt]
                cum = np.concatenate(lists) if lists else np.zeros(0, np.int32)
                offsets = np.cumsum([0] + [len(v) for v in lists]).astype(np.int32)
                fg, area, status = fg_scan(cum, offsets, HW, variant=variant)
                assert not status.any()
                a, b = np.repeat(np.arange(len(dt)), len(gt)), np.tile(np.arange(len(gt)), len(dt)) + len(dt)
                inter, _ = mask_inter((cum, offsets, fg), (cum, offsets, fg), HW, a, b, variant)
                area_det, area_gt = area[:len(dt)], area[len(dt):]
            else:
                boxes = np.asarray([x["box"] for x in dt + gt], np.int64).reshape(-1, 4)
                a, b = np.repeat(np.arange(len(dt)), len(gt)), np.tile(np.arange(len(gt)), len(dt)) + len(dt)
                inter, area_det, area_gt, _ = box_inter(boxes, boxes, a, b)
                area_det, area_gt = ([_area(*[_clamp(v) for v in x["box"]]) for x in part] for part in (dt, gt))
            m, f, status = match([0, len(dt)], [0, len(gt)], [0], inter, np.asarray(area_det, np.int64), np.asarray(area_gt, np.int64),
                                 [int(bool(x["ignore"])) for x in gt], list(thresholds), thr_den, variant)
            assert not status.any()
            groups.append(dict(category=c, scores=[float(x["score"]) for x in dt], dt_match=m, dt_ignore=f,
                               npig=sum(not x["ignore"] for x in gt)))
    return average_precision(groups, thresholds, thr_den, variant)
