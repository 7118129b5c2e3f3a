"""How good a set of 2-D detections is: COCO's average precision over masks ("segm") or boxes ("bbox"), the measure of BOP's
detection and segmentation tasks, with the pairwise work ON the GPU (libgigapose_coco.so, C-ABI: include/gigapose_coco.h, which
spells the arithmetic out; gigapose_testing/coco_ref.py restates it and tests/test_gpu_coco.py holds the kernels to it bit for
bit).  The reference installs pycocotools for this; nothing here needs it.  Masks stay run-length coded: the intersection of two
masks is taken from their runs' prefix sums by binary search, no mask is decoded.

  foreground(masks, HW)                              (cum, offsets) -> Foreground: + fg, area, status          gpc_fg_scan
  mask_intersections(a, b, pair_a, pair_b)           two Foregrounds, P pairs -> inter int64 (P), status      gpc_mask_inter
  box_intersections(box_a, box_b, pair_a, pair_b)    xyxy boxes -> inter, area_a, area_b, status              gpc_box_inter
  match(det_off, gt_off, pair_off, inter, area_det, area_gt, gt_ignore, thresholds, thr_den)
                                                     -> dt_match (T, dets), dt_ignore, status                 gpc_match
  mask_nms(masks, order, num, den)                   -> keep u8: gpc_mask_inter + gpc_sup_bits + the label library's gpa_nms_keep
  average_precision(groups, thresholds, thr_den)     the host half: numpy and Python integers
  DetectionScorer(gts, ...).score(detections)        ground truths of gtinfo.GroundTruthInfo + CNOS dicts -> AP, AP50, AP75, AR
Out of scope: crowd regions, COCO's small / medium / large area ranges, keypoints, float boxes, polygon masks, compressed string
masks, the *_coco.json files, BOP-24's 6-D detection AP.  There is no CPU fallback: a missing library is an error.
"""
import math

import numpy as np
import torch

from . import _lib, proposals
from .ingest import pack_rle

BAD_MASK = 1                                       # status bit of foreground (GPC_BAD_MASK)
PAIR_RANGE, PAIR_MASK = 1, 2                       # of mask_intersections and box_intersections
GROUP_RANGE, GROUP_ORDER, GROUP_SIZE = 1, 2, 4     # of match
MAX_ITEMS_PER_CALL, MAX_THRESHOLDS, MAX_DEN, MAX_GROUP_GT, MAX_NMS = 65535, 16, 65536, 4096, 2048
_coco = _lib.SideLibrary("libgigapose_coco.so", "gpc")
COCO_LIB_PATH, lib, _call = _coco.path, _coco.lib, _coco.call


# ------------------------------------------------------------------------------------------------ the kernels, one wrapper each
class Foreground:
    """Run-length masks with their foreground prefix sums, all on the device: .cum, .offsets (the lists), .fg int32 (total), .area
    int64 (D), .status int32 (D) (BAD_MASK), .HW."""

    def __init__(self, cum, offsets, fg, area, status, HW):
        self.cum, self.offsets, self.fg, self.area, self.status, self.HW = cum, offsets, fg, area, status, HW

    def __len__(self):
        return self.offsets.shape[0] - 1


def _frame(who, HW):
    HW = int(HW)
    if not 0 < HW < 2 ** 31:
        raise ValueError(f"{who}: HW = {HW} pixels (0 < H*W < 2^31)")
    return HW


@torch.no_grad()
def foreground(masks, HW):
    """masks = (cum int32 (total), offsets int32 (D+1)) on the device, as gpi_rle_scan, the string scan and gtinfo's encoder leave
    them (hypotheses.DeviceMasks.lists) -> Foreground.  Any D: chunked at 65535.  A BAD mask (an empty slice, a last prefix sum
    other than HW) has its status bit, area 0, and its part of fg is zero."""
    who = "foreground"
    if not (isinstance(masks, (tuple, list)) and len(masks) == 2):
        raise ValueError(f"{who}: masks must be (cum, offsets)")
    cum, offsets = _lib.arg(masks[0], torch.int32, (None,), who, "cum"), _lib.arg(masks[1], torch.int32, (None,), who, "offsets")
    HW = _frame(who, HW)
    if offsets.shape[0] < 1:
        raise ValueError(f"{who}: offsets holds D + 1 entries, got none")
    _lib.on_gpu(who, cum=cum, offsets=offsets)
    D, dev = offsets.shape[0] - 1, cum.device
    fg = torch.zeros_like(cum)
    area, status = torch.empty(D, dtype=torch.int64, device=dev), torch.empty(D, dtype=torch.int32, device=dev)
    for _, a, b in _lib.chunked(D, MAX_ITEMS_PER_CALL):
        _call("gpc_fg_scan", cum, offsets[a:b + 1], cum.numel(), b - a, HW, fg, area[a:b], status[a:b], _lib.stream_ptr())
    return Foreground(cum, offsets, fg, area, status, HW)


def _pairs(who, pair_a, pair_b):
    pair_a = _lib.arg(pair_a, torch.int32, (None,), who, "pair_a")
    pair_b = _lib.arg(pair_b, torch.int32, (pair_a.shape[0],), who, "pair_b")
    return pair_a, pair_b


@torch.no_grad()
def mask_intersections(masks_a, masks_b, pair_a, pair_b):
    """Two Foregrounds (they may be one), pair_a, pair_b int32 (P) on the device -> (inter int64 (P): the pixels set in both masks
    of a pair, status int32 (P): PAIR_RANGE for an index outside its set, PAIR_MASK for a BAD mask; inter is 0 then).  Any P."""
    who = "mask_intersections"
    if not (isinstance(masks_a, Foreground) and isinstance(masks_b, Foreground)):
        raise ValueError(f"{who}: masks_a and masks_b must be Foregrounds (detections.foreground makes them)")
    if masks_a.HW != masks_b.HW:
        raise ValueError(f"{who}: the two sets lie on frames of {masks_a.HW} and {masks_b.HW} pixels")
    pair_a, pair_b = _pairs(who, pair_a, pair_b)
    _lib.on_gpu(who, pair_a=pair_a, pair_b=pair_b)
    P, dev = pair_a.shape[0], pair_a.device
    inter, status = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    A, B = masks_a, masks_b
    for _, a, b in _lib.chunked(P, MAX_ITEMS_PER_CALL):
        _call("gpc_mask_inter", A.cum, A.offsets, A.fg, A.cum.numel(), len(A), B.cum, B.offsets, B.fg, B.cum.numel(), len(B), A.HW, pair_a[a:b], pair_b[a:b],
              b - a, inter[a:b], status[a:b], _lib.stream_ptr())
    return inter, status


@torch.no_grad()
def box_intersections(box_a, box_b, pair_a, pair_b):
    """box_a (DA, 4), box_b (DB, 4) int32 xyxy with exclusive ends, pair_a, pair_b int32 (P), on the device -> (inter, area_a,
    area_b int64 (P), status int32 (P)); coordinates are clamped to [-2^21, 2^21].  Any P."""
    who = "box_intersections"
    box_a, box_b = _lib.arg(box_a, torch.int32, (None, 4), who, "box_a"), _lib.arg(box_b, torch.int32, (None, 4), who, "box_b")
    pair_a, pair_b = _pairs(who, pair_a, pair_b)
    _lib.on_gpu(who, box_a=box_a, box_b=box_b, pair_a=pair_a, pair_b=pair_b)
    P, dev = pair_a.shape[0], pair_a.device
    inter, area_a, area_b = (torch.empty(P, dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.empty(P, dtype=torch.int32, device=dev)
    for _, a, b in _lib.chunked(P, MAX_ITEMS_PER_CALL):
        _call("gpc_box_inter", box_a, box_a.shape[0], box_b, box_b.shape[0], pair_a[a:b], pair_b[a:b], b - a, inter[a:b], area_a[a:b], area_b[a:b], status[a:b],
              _lib.stream_ptr())
    return inter, area_a, area_b, status


def _thresholds(who, thresholds, thr_den):
    nums, den = [int(v) for v in thresholds], int(thr_den)
    if not 1 <= len(nums) <= MAX_THRESHOLDS:
        raise ValueError(f"{who}: {len(nums)} thresholds (1 to {MAX_THRESHOLDS})")
    if not (1 <= den <= MAX_DEN and all(0 <= n <= den for n in nums)):
        raise ValueError(f"{who}: bad IoU thresholds {nums} / {den} (integers, 0 <= num <= den, 1 <= den <= 2^16)")
    return nums, den


@torch.no_grad()
def match(det_off, gt_off, pair_off, inter, area_det, area_gt, gt_ignore, thresholds, thr_den):
    """COCO's greedy matching (include/gigapose_coco.h: gpc_match).  Q groups, one per (image, category): det_off, gt_off int32
    (Q+1), pair_off int32 (Q), inter int64 (pairs): group q's D_q x G_q block, row-major, at pair_off[q]; area_det int64 (dets),
    area_gt int64 (gts), gt_ignore u8 (gts); all on the device.  A group's detections stand best first, its non-ignored ground
    truths before its ignored ones.  thresholds: T numerators over thr_den.
    -> (dt_match int32 (T, dets): the ground truth's index within its group or -1, dt_ignore u8 (T, dets), status int32 (Q)).
    A group with GROUP_RANGE leaves its entries at -1 / 0.  Any Q: chunked at 65535."""
    who = "match"
    nums, den = _thresholds(who, thresholds, thr_den)
    det_off, gt_off = _lib.arg(det_off, torch.int32, (None,), who, "det_off"), _lib.arg(gt_off, torch.int32, (None,), who, "gt_off")
    Q = det_off.shape[0] - 1
    if Q < 0 or gt_off.shape[0] != Q + 1:
        raise ValueError(f"{who}: det_off and gt_off hold Q + 1 entries each, got {det_off.shape[0]} and {gt_off.shape[0]}")
    pair_off = _lib.arg(pair_off, torch.int32, (Q,), who, "pair_off")
    inter, area_det = _lib.arg(inter, torch.int64, (None,), who, "inter"), _lib.arg(area_det, torch.int64, (None,), who, "area_det")
    area_gt = _lib.arg(area_gt, torch.int64, (None,), who, "area_gt")
    gt_ignore = _lib.arg(gt_ignore, torch.uint8, (area_gt.shape[0],), who, "gt_ignore")
    _lib.on_gpu(who, det_off=det_off, gt_off=gt_off, pair_off=pair_off, inter=inter, area_det=area_det, area_gt=area_gt, gt_ignore=gt_ignore)
    dev, TD, T = det_off.device, area_det.shape[0], len(nums)
    thr = torch.tensor(nums, dtype=torch.int32, device=dev)
    dt_match = torch.full((T, TD), -1, dtype=torch.int32, device=dev)
    dt_ignore = torch.zeros((T, TD), dtype=torch.uint8, device=dev)
    status = torch.empty(Q, dtype=torch.int32, device=dev)
    for _, a, b in _lib.chunked(Q, MAX_ITEMS_PER_CALL):
        _call("gpc_match", det_off[a:b + 1], gt_off[a:b + 1], pair_off[a:b], b - a, inter, inter.shape[0], area_det, TD, area_gt, gt_ignore, area_gt.shape[0],
              thr, T, den, dt_match, dt_ignore, status[a:b], _lib.stream_ptr())
    return dt_match, dt_ignore, status


@torch.no_grad()
def sup_bits(inter, area, num, den):
    """inter int64 (P, P) (read above the diagonal), area int64 (P), in suppression order, on the device -> sup int64 (P, (P + 63)
    // 64): bit j of row i set iff j > i and inter * den > num * union -- what proposals.nms_keep takes.  P <= 2048."""
    who = "sup_bits"
    area = _lib.arg(area, torch.int64, (None,), who, "area")
    P = area.shape[0]
    inter = _lib.arg(inter, torch.int64, (P, P), who, "inter")
    num, den = proposals._threshold((num, den))
    if P > MAX_NMS:
        raise ValueError(f"{who}: {P} masks in one call (the limit is {MAX_NMS})")
    _lib.on_gpu(who, inter=inter, area=area)
    sup = torch.empty(P, (P + 63) // 64, dtype=torch.int64, device=area.device)
    _call("gpc_sup_bits", inter, area, P, num, den, sup, _lib.stream_ptr())
    return sup


@torch.no_grad()
def mask_nms(masks, order, num, den, label=None):
    """masks: a Foreground; order int64 (P) on the device: the masks to compare, best first -> keep u8 (P): mask order[j] goes
    when a KEPT order[i], i < j, has mask IoU > num / den with it (on integers: inter * den > num * union).  All pairs i < j go
    through mask_intersections, then gpc_sup_bits, then the greedy pass of the box NMS (proposals.nms_keep).  label int32 (D) or
    None: with labels, only masks of one label suppress each other.  P <= 2048."""
    who = "mask_nms"
    if not isinstance(masks, Foreground):
        raise ValueError(f"{who}: masks must be a Foreground (detections.foreground makes it)")
    order = _lib.arg(order, torch.int64, (None,), who, "order")
    num, den = proposals._threshold((num, den))
    P = order.shape[0]
    if P > MAX_NMS:
        raise ValueError(f"{who}: {P} masks in one call (the limit is {MAX_NMS})")
    if label is not None:
        label = _lib.arg(label, torch.int32, (len(masks),), who, "label")
        _lib.on_gpu(who, label=label)
    _lib.on_gpu(who, order=order)
    dev = order.device
    i, j = torch.triu_indices(P, P, 1, device=dev)
    a, b = order[i].to(torch.int32), order[j].to(torch.int32)
    part, status = mask_intersections(masks, masks, a, b)
    if label is not None:
        part = torch.where(label[a.long()] == label[b.long()], part, torch.zeros_like(part))
    inter = torch.zeros(P, P, dtype=torch.int64, device=dev)
    inter[i, j] = part
    safe = order.clamp(0, max(len(masks) - 1, 0))
    keep = proposals.nms_keep(sup_bits(inter, masks.area[safe] if len(masks) else torch.zeros(P, dtype=torch.int64, device=dev), num, den))
    flagged = int(status.max()) if status.numel() else 0
    if flagged or (P and (int(order.min()) < 0 or int(order.max()) >= len(masks))):
        raise ValueError(f"{who}: a mask of `order` lies outside the set or is a bad list (pair status {flagged})")
    return keep


# ------------------------------------------------------------------------------------------------ the host half: AP
def _mean(values):
    values = list(values)
    return math.fsum(values) / len(values) if values else -1.0


def average_precision(groups, thresholds, thr_den):
    """COCO's average precision over matched detections, in numpy and Python integers.

    groups: per (image, category), IN IMAGE ORDER, a dict(category, scores (D) floats, dt_match (T, D): >= 0 where matched,
    dt_ignore (T, D), npig: the number of non-ignored ground truths); every image already cut to its max_dets.  thresholds: the T
    numerators over thr_den (AP50 and AP75 are the thresholds equal to 1/2 and 3/4).
    Per category and threshold (a CELL): the detections of all images in image order, sorted stably by score, descending; the
    ignored ones dropped; tp, fp their cumulative counts.  For each recall level i / 100, i = 0 .. 100, the first rank with
    100 * tp >= i * npig (an integer comparison); the precision there is tp / (tp + fp), ONE float64 division, after the
    precisions have been made non-increasing from the right; past the last rank it is 0.  The cell's AP is math.fsum of the 101
    values / 101, its recall the last tp / npig (0 without detections).  Cells with npig == 0 are left out.
    -> dict(AP, AP50, AP75, AR: means (math.fsum / count) over the cells, -1.0 over none; per_category {category: the same four};
    cells {(category, t): (ap, recall)}).
    Where this departs from pycocotools: no epsilon is added to the denominator tp + fp; the IoU thresholds are exact rationals
    (n / 20), not numpy.linspace's doubles, and the recall levels are compared on integers; so only exact ties -- an IoU or a
    recall exactly at a level -- can fall differently.  It has not been compared with pycocotools itself."""
    nums, den = _thresholds("average_precision", thresholds, thr_den)
    T = len(nums)
    levels = np.arange(101, dtype=np.int64)
    cells = {}
    for c in sorted({g["category"] for g in groups}):
        mine = [g for g in groups if g["category"] == c]
        npig = sum(int(g["npig"]) for g in mine)
        if npig == 0:
            continue
        scores = np.concatenate([np.asarray(g["scores"], np.float64).reshape(-1) for g in mine])
        if np.isnan(scores).any():
            raise ValueError(f"average_precision: a score of category {c} is NaN")
        matched = np.concatenate([np.asarray(g["dt_match"]).reshape(T, -1) >= 0 for g in mine], axis=1)
        ignored = np.concatenate([np.asarray(g["dt_ignore"]).reshape(T, -1) != 0 for g in mine], axis=1)
        if matched.shape[1] != len(scores) or ignored.shape[1] != len(scores):
            raise ValueError(f"average_precision: category {c}: {len(scores)} scores for {matched.shape[1]} matches")
        order = np.argsort(-scores, kind="stable")
        for t in range(T):
            counted = ~ignored[t][order]
            hit = matched[t][order][counted]
            tp, fp = np.cumsum(hit, dtype=np.int64), np.cumsum(~hit, dtype=np.int64)
            prec = np.maximum.accumulate((tp / (tp + fp))[::-1])[::-1]       # a correctly rounded division is monotone: the float
            rank = np.searchsorted(100 * tp, levels * npig, side="left")      # envelope is the division of the rational one
            values = np.where(rank < len(tp), prec[np.minimum(rank, max(len(tp) - 1, 0))] if len(tp) else 0.0, 0.0)
            cells[(c, t)] = (math.fsum(values.tolist()) / 101, int(tp[-1]) / npig if len(tp) else 0.0)
    at = {name: [t for t, n in enumerate(nums) if n * q == p * den] for name, (p, q) in (("AP50", (1, 2)), ("AP75", (3, 4)))}

    def table(keys):
        return dict(AP=_mean(cells[k][0] for k in keys), AR=_mean(cells[k][1] for k in keys),
                    **{name: _mean(cells[k][0] for k in keys if k[1] in ts) for name, ts in at.items()})

    keys = sorted(cells)
    out = table(keys)
    out["per_category"] = {c: table([k for k in keys if k[0] == c]) for c in sorted({k[0] for k in keys})}
    out["cells"] = cells
    return out


# ------------------------------------------------------------------------------------------------ the scorer
def _xywh_box(who, what, bbox):
    v = [float(x) for x in bbox]
    if len(v) != 4 or any(x != x or x != math.floor(x) or abs(x) > 2 ** 21 for x in v):
        raise ValueError(f"{who}: {what} has the box {list(bbox)}: only integral xywh boxes within 2^21 are scored (float boxes are out of scope)")
    x, y, w, h = (int(x) for x in v)
    if max(w, 0) * max(h, 0) >= 2 ** 31:
        raise ValueError(f"{who}: {what} has the box {list(bbox)}: its area must stay below 2^31")
    return [x, y, x + w, y + h]


class DetectionScorer:
    """COCO AP of detections against the ground truths of a set of images.

    gts: a gtinfo.GroundTruthTable from GroundTruthInfo.compute(gts, masks=True) -- its masks stay on the device, nothing is packed
    or scanned again -- or a plain {(scene_id, im_id): [rows]} of the same rows, whose "mask" / "mask_visib" hold uncompressed
    `counts` on the host (they go through ingest.pack_rle and gpi_rle_scan).  A row's category is its "obj_id" (or
    "category_id"); GroundTruthInfo's rows carry none, so `objects` = the {(scene_id, im_id): [{"obj_id", ...}]} that compute
    was given names them.
    iou_type "segm": the IoU of the masks; "bbox": of the boxes "bbox_visib" (gt_mask="mask_visib") or "bbox_obj" ("mask").
    min_visib: a ground truth whose "visib_fract" is below it is IGNORED -- it does not count as missed, and a detection matched
    to it counts neither as true nor as false (None: nothing is ignored; a number needs "visib_fract" on every row).
    max_dets: per image and category, the best that many detections are scored.  thresholds / thr_den: the IoU thresholds as
    exact rationals (COCO: 10/20 .. 19/20).

    .score(detections), detections {(scene_id, im_id): [CNOS dicts {"category_id", "score", "bbox" xywh, "segmentation"}]} -- what
    ProposalLabeller.label returns per image and FrameIngest takes -> the dictionary of average_precision.  "segm" needs the
    uncompressed `segmentation` (a compressed string raises, as ingest.pack_rle does); "bbox" needs integral boxes.  Images are taken
    in sorted key order.  An image that only the detections name has no ground truths: its detections are false positives."""

    def __init__(self, gts, iou_type="segm", gt_mask="mask_visib", min_visib=0.1, max_dets=100, thresholds=tuple(range(10, 20)), thr_den=20,
                 device="cuda", objects=None):
        who = "DetectionScorer"
        if iou_type not in ("segm", "bbox"):
            raise ValueError(f"{who}: iou_type must be 'segm' or 'bbox', got {iou_type!r}")
        if gt_mask not in ("mask_visib", "mask"):
            raise ValueError(f"{who}: gt_mask must be 'mask_visib' or 'mask', got {gt_mask!r}")
        if min_visib is not None and not 0 <= float(min_visib) <= 1:
            raise ValueError(f"{who}: min_visib must be None or lie in [0, 1], got {min_visib!r}")
        if int(max_dets) < 1:
            raise ValueError(f"{who}: max_dets = {max_dets}")
        self.iou_type, self.gt_mask, self.max_dets, self.device = iou_type, gt_mask, int(max_dets), torch.device(device)
        self.min_visib = None if min_visib is None else float(min_visib)
        self.thresholds, self.thr_den = _thresholds(who, thresholds, thr_den)
        rows = []                                                     # (image key, category, ignore, the row) in the table's order
        keys = getattr(gts, "instances", None) or [(k[0], k[1], j) for k, listed in gts.items() for j in range(len(listed))]
        for s, im, j in keys:
            row = gts[(s, im)][j]
            cat = row.get("obj_id", row.get("category_id"))
            if cat is None and objects is not None:
                named = objects.get((s, im), [])
                if len(named) != len(gts[(s, im)]):
                    raise ValueError(f"{who}: image {(s, im)} lists {len(gts[(s, im)])} ground truths and `objects` {len(named)}")
                cat = named[j]["obj_id"]
            if cat is None:
                raise ValueError(f"{who}: a ground truth of image {(s, im)} has no 'obj_id' (pass objects=, the ground truths compute was given)")
            if self.min_visib is not None and row.get("visib_fract") is None:
                raise ValueError(f"{who}: min_visib is set and a ground truth of object {cat} has no 'visib_fract' (gtinfo.with_visibility adds it)")
            rows.append(((int(s), int(im)), int(cat), self.min_visib is not None and float(row["visib_fract"]) < self.min_visib, row))
        self.rows = rows
        self.size = None
        self.gt_fg = self.gt_box = None
        if iou_type == "bbox":
            name = "bbox_visib" if gt_mask == "mask_visib" else "bbox_obj"
            self.gt_box_host = np.asarray([_xywh_box(who, f"a ground truth of image {r[0]}", r[3][name]) for r in rows], np.int32).reshape(-1, 4)
            return
        device_masks = getattr(gts, "masks_visib" if gt_mask == "mask_visib" else "masks", None)
        if device_masks is not None:
            self.size = tuple(device_masks.size)
            self._gt_lists = device_masks.lists
        else:
            segs = [r[3].get(gt_mask) for r in rows]
            if any(s is None for s in segs):
                raise ValueError(f"{who}: a ground truth has no '{gt_mask}' (GroundTruthInfo.compute(gts, masks=True) adds it)")
            self.size = tuple(int(v) for v in segs[0]["size"]) if segs else None
            self._gt_lists = None
            self._gt_packed = pack_rle(segs, *self.size) if segs else None

    def _ground_truth_masks(self, who):
        if self.gt_fg is None:
            H, W = self.size
            if self._gt_lists is None:
                cum, offsets, check = proposals.scan_lists(who, *self._gt_packed, H, W, self.device)
                check()
                self._gt_lists = (cum, offsets)
            self.gt_fg = foreground(self._gt_lists, H * W)
            if int(self.gt_fg.status.max()) if len(self.gt_fg) else 0:
                raise ValueError(f"{who}: a ground truth's mask is a bad run-length list")
        return self.gt_fg

    @torch.no_grad()
    def score(self, detections):
        who = "DetectionScorer.score"
        segm = self.iou_type == "segm"
        by_image = {}
        for n, (key, cat, ignore, _) in enumerate(self.rows):
            by_image.setdefault(key, {}).setdefault(cat, []).append((ignore, n))
        dets_of = {}
        for key, listed in detections.items():
            for n, d in enumerate(listed):
                score = float(d["score"])
                if score != score:
                    raise ValueError(f"{who}: detection {n} of image {tuple(key)} has a NaN score")
                dets_of.setdefault((int(key[0]), int(key[1])), {}).setdefault(int(d["category_id"]), []).append((score, n, d))
        groups, det_items, gt_index = [], [], []                       # groups: (category, its detections, its (ignore, row index) pairs)
        for key in sorted(set(by_image) | set(dets_of)):
            for cat in sorted(set(by_image.get(key, {})) | set(dets_of.get(key, {}))):
                dt = sorted(dets_of.get(key, {}).get(cat, []), key=lambda x: -x[0])[:self.max_dets]      # stable: ties in input order
                gt = sorted(by_image.get(key, {}).get(cat, []), key=lambda x: x[0])                       # the ignored ones last
                if len(gt) > MAX_GROUP_GT:
                    raise ValueError(f"{who}: image {key} has {len(gt)} ground truths of category {cat} (at most {MAX_GROUP_GT})")
                groups.append((key, cat, dt, gt))
                det_items += [(key, n, d) for _, n, d in dt]
                gt_index += [n for _, n in gt]
        if segm:                                                      # everything the host can refuse, before the device is needed
            if any(d.get("segmentation") is None for _, _, d in det_items):
                raise ValueError(f"{who}: iou_type 'segm' needs every detection's 'segmentation'")
            if self.size is None and det_items:
                self.size = tuple(int(v) for v in det_items[0][2]["segmentation"]["size"])
            H, W = self.size if self.size is not None else (1, 1)
            counts, offsets = pack_rle([d["segmentation"] for _, _, d in det_items], H, W)
        else:
            det_box_host = np.asarray([_xywh_box(who, f"detection {n} of image {key}", d["bbox"]) for key, n, d in det_items], np.int32).reshape(-1, 4)
        if self.device.type != "cuda":
            raise _lib.GigaPoseHipError(f"{who} needs a GPU device (no CPU fallback)")
        dev = self.device
        D = np.asarray([len(g[2]) for g in groups], np.int64)
        G = np.asarray([len(g[3]) for g in groups], np.int64)
        det_off, gt_off = np.concatenate(([0], np.cumsum(D))), np.concatenate(([0], np.cumsum(G)))
        pair_off = np.concatenate(([0], np.cumsum(D * G)))
        if pair_off[-1] >= 2 ** 31:
            raise ValueError(f"{who}: {int(pair_off[-1])} pairs of detections and ground truths (the lists are indexed with 32 bits: score fewer images per call)")
        pair_a = np.concatenate([np.repeat(np.arange(det_off[q], det_off[q + 1]), G[q]) for q in range(len(groups))] + [np.zeros(0, np.int64)])
        pair_b = np.concatenate([np.tile(np.asarray(gt_index[gt_off[q]:gt_off[q + 1]], np.int64), D[q]) for q in range(len(groups))] + [np.zeros(0, np.int64)])
        to_dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)      # noqa: E731
        pair_a_d, pair_b_d = to_dev(pair_a, torch.int32), to_dev(pair_b, torch.int32)
        gt_sel = to_dev(np.asarray(gt_index, np.int64), torch.int64)
        if segm:
            cum, offsets_d, check = proposals.scan_lists(who, counts, offsets, H, W, dev)
            check()
            det_fg = foreground((cum, offsets_d), H * W)
            gt_fg = self._ground_truth_masks(who) if self.rows else foreground((torch.zeros(0, dtype=torch.int32, device=dev),
                                                                                 torch.zeros(1, dtype=torch.int32, device=dev)), H * W)
            inter, status = mask_intersections(det_fg, gt_fg, pair_a_d, pair_b_d)
            area_det, area_gt = det_fg.area, gt_fg.area[gt_sel]
        else:
            det_box = to_dev(det_box_host, torch.int32)
            if self.gt_box is None:
                self.gt_box = to_dev(self.gt_box_host, torch.int32)
            inter, _, _, status = box_intersections(det_box, self.gt_box, pair_a_d, pair_b_d)
            every = torch.arange(det_box.shape[0], dtype=torch.int32, device=dev)
            area_det = box_intersections(det_box, det_box, every, every)[1]
            area_gt = box_intersections(self.gt_box, self.gt_box, gt_sel.to(torch.int32), gt_sel.to(torch.int32))[1]
        ignore = to_dev(np.asarray([self.rows[n][2] for n in gt_index], np.uint8), torch.uint8)
        dt_match, dt_ignore, gstatus = match(to_dev(det_off, torch.int32), to_dev(gt_off, torch.int32), to_dev(pair_off[:-1], torch.int32), inter,
                                             area_det.contiguous(), area_gt.contiguous(), ignore, self.thresholds, self.thr_den)
        if (int(status.max()) if status.numel() else 0) or (int(gstatus.max()) if gstatus.numel() else 0):
            raise _lib.GigaPoseHipError(f"{who}: the kernels flag a pair or a group (pair status {int(status.max()) if status.numel() else 0}, "
                                        f"group status {int(gstatus.max()) if gstatus.numel() else 0})")
        m, f = dt_match.cpu().numpy(), dt_ignore.cpu().numpy()
        records = [dict(category=cat, scores=[x[0] for x in dt], dt_match=m[:, det_off[q]:det_off[q + 1]], dt_ignore=f[:, det_off[q]:det_off[q + 1]],
                        npig=sum(not ig for ig, _ in gt)) for q, (_, cat, dt, gt) in enumerate(groups)]
        return average_precision(records, self.thresholds, self.thr_den)
