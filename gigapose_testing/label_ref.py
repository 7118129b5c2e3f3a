"""include/gigapose_label.h restated in numpy and Python integers: what libgigapose_label.so (gigapose_amd/proposals.py) is held
to bit for bit (tests/test_gpu_label.py), and what tests/test_label_host.py holds to readings that cannot share its mistakes.

  descriptors(x, gamma, beta, eps)           the header's summation order in float64, numpy.sqrt for the two roots
  scores(q, bank, k)                         int64 products and sums; sorted top-k; first maxima
  run_boxes(cum, offsets, total, H, W)       one run of ones at a time
  nms_matrix(box, label, num, den, ...)      Python integers;  nms_keep(sup): the textbook loop
  label_proposals(...)                       the labeller's decisions after the scores: drop, order, suppress, cut
`variant` names a subtly wrong version (VARIANTS); the host tests show that each of them fails a check."""
import numpy as np

Q_BITS = 20
Q_ONE = 1 << Q_BITS
THREADS = 256
NON_FINITE, ZERO_NORM = 1, 2
EMPTY_MASK, BAD_MASK = 1, 2
MAX_COORD = 1 << 21
VARIANTS = ("last_maximum", "k_not_min", "abs_topk", "iou_not_strict", "suppressed_suppress", "inclusive_x1", "one_column")


# ------------------------------------------------------------------------------------------------ descriptors
def block_sum(v):
    """SUM of the header over the last axis of v (.., C) float64: thread t adds v[t], v[t + 256], .. in order to +0.0, then the
    pairwise tree over the 256 partials."""
    C = v.shape[-1]
    part = np.zeros(v.shape[:-1] + (THREADS,), np.float64)
    for c0 in range(0, C, THREADS):
        n = min(THREADS, C - c0)
        part[..., :n] = part[..., :n] + v[..., c0:c0 + n]
    off = THREADS // 2
    while off >= 1:
        part = part[..., :off] + part[..., off:2 * off]
        off //= 2
    return part[..., 0]


def descriptors(x, gamma, beta, eps):
    """x (B, C) f32 class tokens -> (q int32 (B, C), status int32 (B))."""
    x = np.asarray(x, np.float32).astype(np.float64)
    g, b = np.asarray(gamma, np.float32).astype(np.float64), np.asarray(beta, np.float32).astype(np.float64)
    B, C = x.shape
    with np.errstate(all="ignore"):
        mean = block_sum(x) / np.float64(C)
        dev = x - mean[:, None]
        var = block_sum(dev * dev) / np.float64(C)
        r = np.float64(1.0) / np.sqrt(var + np.float64(eps))
        y = (dev * r[:, None]) * g + b
        n2 = block_sum(y * y)
        status = np.zeros(B, np.int32)
        status[n2 == 0] = ZERO_NORM
        status[~np.isfinite(x).all(axis=1) | ~np.isfinite(n2)] = NON_FINITE
        norm = np.where(status != 0, 1.0, np.sqrt(n2))
        q = np.rint((y / norm[:, None]) * np.float64(Q_ONE))
    q[status != 0] = 0
    return q.astype(np.int32), status


# ------------------------------------------------------------------------------------------------ scores
def dots(q, bank):
    """q (P, C), bank (O, T, C) integers -> dot (P, O, T) int64, exact."""
    q, bank = np.asarray(q, np.int64), np.asarray(bank, np.int64)
    O, T, C = bank.shape
    return (q @ bank.reshape(O * T, C).T).reshape(q.shape[0], O, T)


def _first_max(v, last=False):
    v = np.asarray(v)
    return int(len(v) - 1 - np.argmax(v[::-1])) if last else int(np.argmax(v))


def scores(q, bank, k, variant=None):
    """-> dict(dot (P,O,T), obj (P,O), label (P), score (P), best_template (P), kk)."""
    dot = dots(q, bank)
    P, O, T = dot.shape
    kk = k if variant == "k_not_min" else min(k, T)             # the wrong version divides a sum of T < k dots by k
    if variant == "abs_topk":
        order = np.argsort(-np.abs(dot), axis=2, kind="stable")[:, :, :kk]
        obj = np.take_along_axis(dot, order, axis=2).sum(axis=2)
    else:
        obj = (-np.sort(-dot, axis=2)[:, :, :kk]).sum(axis=2)
    last = variant == "last_maximum"
    label = np.asarray([_first_max(obj[p], last) for p in range(P)], np.int32).reshape(P)
    score = obj[np.arange(P), label] if P else np.zeros(0, np.int64)
    best = np.asarray([_first_max(dot[p, label[p]], last) for p in range(P)], np.int32).reshape(P)
    return dict(dot=dot, obj=obj.astype(np.int64), label=label, score=score.astype(np.int64), best_template=best, kk=kk)


def float_score(score, kk):
    """The int64 sum as the float64 mean cosine: one correctly rounded division (both operands are exact doubles)."""
    return np.asarray(score, np.int64).astype(np.float64) / np.float64(kk * (1 << (2 * Q_BITS)))


# ------------------------------------------------------------------------------------------------ boxes
def run_boxes(cum, offsets, total, H, W, variant=None):
    """-> (box int32 (D,4), area int64 (D), status int32 (D))."""
    cum, offsets = np.asarray(cum, np.int64), np.asarray(offsets, np.int64)
    D, HW = len(offsets) - 1, H * W
    box, area, status = np.zeros((D, 4), np.int32), np.zeros(D, np.int64), np.zeros(D, np.int32)
    for d in range(D):
        lo, hi = int(offsets[d]), int(offsets[d + 1])
        if not (0 <= lo < hi <= total) or cum[hi - 1] != HW:
            status[d] = BAD_MASK
            continue
        x0 = y0 = None
        x1 = y1 = n = 0
        for i in range(lo + 1, hi, 2):
            a, b = int(cum[i - 1]), int(cum[i])
            if not (0 <= a < b <= HW):
                continue
            xa, ya, xb, yb = a // H, a % H, (b - 1) // H, (b - 1) % H
            n += b - a
            x0 = xa if x0 is None else min(x0, xa)
            x1 = max(x1, xb + (0 if variant == "inclusive_x1" else 1))
            if xa == xb or variant == "one_column":
                lo_y, hi_y = (ya, yb + 1) if xa == xb else (min(ya, yb), max(ya, yb) + 1)
            else:
                lo_y, hi_y = 0, H
            y0 = lo_y if y0 is None else min(y0, lo_y)
            y1 = max(y1, hi_y)
        if n == 0:
            status[d] = EMPTY_MASK
            continue
        box[d], area[d] = (x0, y0, x1, y1), n
    return box, area, status


# ------------------------------------------------------------------------------------------------ NMS
def _area(x0, y0, x1, y1):
    return np.maximum(0, x1 - x0) * np.maximum(0, y1 - y0)


def suppression(box, label, num, den, per_label, variant=None):
    """-> bool (P, P): [i, j] is True iff box i suppresses box j.  int64 throughout: every product stays below 2^62."""
    b = np.clip(np.asarray(box, np.int64).reshape(-1, 4), -MAX_COORD, MAX_COORD)
    P = len(b)
    area = _area(b[:, 0], b[:, 1], b[:, 2], b[:, 3])
    out = np.zeros((P, P), bool)
    for i in range(P):
        inter = _area(np.maximum(b[i, 0], b[:, 0]), np.maximum(b[i, 1], b[:, 1]), np.minimum(b[i, 2], b[:, 2]), np.minimum(b[i, 3], b[:, 3]))
        union = area[i] + area - inter
        hit = inter * den >= num * union if variant == "iou_not_strict" else inter * den > num * union
        if per_label:
            hit &= np.asarray(label) == label[i]
        hit[:i + 1] = False
        out[i] = hit
    return out


def nms_matrix(box, label, num, den, per_label, variant=None):
    """-> sup (P, words) uint64: bit (j & 63) of word j / 64 of row i."""
    hit = suppression(box, label, num, den, per_label, variant)
    P = len(hit)
    words = (P + 63) // 64
    padded = np.zeros((P, words * 64), np.uint64)
    padded[:, :P] = hit
    return (padded.reshape(P, words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(P, words)


def nms_keep(sup, P, variant=None):
    """The textbook loop -> keep uint8 (P)."""
    sup = np.asarray(sup, np.uint64).reshape(P, (P + 63) // 64)
    hit = ((sup[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(P, sup.shape[1] * 64)[:, :P]
    gone, keep = np.zeros(P, bool), np.zeros(P, np.uint8)
    for i in range(P):
        if gone[i] and variant != "suppressed_suppress":
            continue
        keep[i] = not gone[i]
        gone |= hit[i]
    return keep


def nms(box, label, num, den, per_label, variant=None):
    box = np.asarray(box).reshape(-1, 4)
    return nms_keep(nms_matrix(box, label, num, den, per_label, variant), len(box), variant)


# ------------------------------------------------------------------------------------------------ the labeller's decisions
def label_proposals(image_of, sc, dstatus, mstatus, box, top_k_used, min_score, nms_iou, per_label, max_dets, n_img):
    """What ProposalLabeller.label decides once the scores are there.  image_of (P) the frame of a proposal, sc: scores()'s dict
    (or its fields from the device), dstatus / mstatus (P) the descriptor and mask flags, box (P,4) xyxy
    -> (per image the kept proposal indices in output order, report dict)."""
    P = len(image_of)
    fscore = float_score(sc["score"], top_k_used)
    report = dict(proposals=P, empty_mask=0, flagged_descriptor=0, low_score=0, suppressed=0, over_max_dets=0, kept=0)
    out = []
    for im in range(n_img):
        alive = []
        for p in (int(v) for v in np.flatnonzero(np.asarray(image_of) == im)):
            if mstatus[p]:
                report["empty_mask"] += 1
            elif dstatus[p]:
                report["flagged_descriptor"] += 1
            elif fscore[p] < min_score:
                report["low_score"] += 1
            else:
                alive.append(p)
        alive.sort(key=lambda p: (-int(sc["score"][p]), p))
        keep = nms([box[p] for p in alive], [sc["label"][p] for p in alive], nms_iou[0], nms_iou[1], per_label)
        kept = [p for p, kp in zip(alive, keep) if kp]
        report["suppressed"] += len(alive) - len(kept)
        if max_dets is not None and len(kept) > max_dets:
            report["over_max_dets"] += len(kept) - max_dets
            kept = kept[:max_dets]
        report["kept"] += len(kept)
        out.append(kept)
    return out, report
