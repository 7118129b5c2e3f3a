"""Choosing among a detection's pose hypotheses ON the GPU: how well each one, drawn, fits the sensor's depth and the detection's
mask (libgigapose_verify.so, C-ABI: include/gigapose_verify.h, which spells the arithmetic out; gigapose_testing/verify_ref.py
restates it in numpy and tests/test_gpu_verify.py holds the kernel to it bit for bit).  The path ends in two csv files, the top-1
file and `...MultiHypothesis.csv` with k = 5 hypotheses per detection and an `instance_id`; the reference's refiners consume the
second (n_pose_hypotheses: 5, src/megapose/utils/load_model.py:27-45), refine all five and keep the one that fits the image best
-- which is how a wrong nearest template is recovered from.  This module is that last step with the parts the project has: a
hypothesis is drawn by the compute rasteriser (render.project + render.raster: a z-buffer of 64-bit keys) and gpv_counts counts,
over its box, the pixels whose measured depth agrees with the drawn one, lies BEHIND it (the sensor sees through the drawn
surface: a free-space violation) or in FRONT of it (an occluder, or a contradiction), each inside and outside the detection's
run-length mask, which stays on the device as the ingest library's prefix sums.  Integer counts: their bits depend on no
summation order.

  counts(vis, depth, frame, masks, det, box, tol)  -> counts int64 (N,16), status int32 (N,)
  verification_scores(counts, mask_area, ...)      -> {"verify", "depth_fit", "iou", "residual"}: host, float64
  read_hypotheses(path)                            evaluate.read_estimates + "instance_id"
  HypothesisVerifier(models, cameras, ...)         .score(estimates, masks)  .select(...)  .rank(...)
  refine_and_select(refiner, verifier, estimates, masks)   csv -> refine -> select -> csv -> PoseScorer.score_csv
Out of scope: nearest-neighbour association, colour or edge terms, the MegaPose scorer network, a learned combination of the
two scores, polygon segmentations; a view that the near plane clips scores 0.  There is no CPU fallback: a missing library is an
error.
"""
import numpy as np
import torch

from . import _lib, refine
from .evaluate import read_estimates
from .hypotheses import MAX_PAIRS_PER_CALL, MAX_PIXELS, DeviceMasks, HypothesisFlow, mask_lists, need_gpu, pack_masks, scan_masks  # (gigapose_verify.h: Limits)

COUNTS = 16
UNMEASURED, AGREE, BEHIND, FRONT = 0, 1, 2, 3        # a covered pixel's class: counts[2*class + in_mask]
UNCOVERED_IN_MASK, RESIDUAL = 8, 9
QUANTUM_BITS = 20
BAD_FRAME, BAD_MASK = 1, 2
STATUS_BITS = {BAD_FRAME: "the frame index lies outside the depth stack", BAD_MASK: "the detection index or its run-length list is bad"}
_verify = _lib.SideLibrary("libgigapose_verify.so", "gpv")
VERIFY_LIB_PATH, lib, _call = _verify.path, _verify.lib, _verify.call


def pixels_per_workgroup():
    return int(lib().gpv_pixels_per_workgroup())


@torch.no_grad()
def counts(vis, depth, frame, masks, det, box, tol, out=None):
    """gpv_counts: vis int64 (N,H,W) holding render.raster's keys; depth f32 (M,H,W) or None (then frame is not read and may be
    None); frame int32 (N,); masks None or (cum, offsets), int32 (total,) and (D+1,) as ingest.RleDetectionPreprocessor.scan
    returns them; det int32 (N,) into D, -1 = no mask for the pair (not read and may be None without masks); box int32 (N,4) x0
    y0 x1 y1 inclusive; tol f64 (N,), all on the device -> counts int64 (N,16), status int32 (N,) on the device.  N <= 65535,
    H*W <= 2^22.  `out` = (counts, status) are buffers to write into."""
    who = "counts"
    vis = _lib.arg(vis, torch.int64, (None, None, None), who, "vis")
    N, H, W = vis.shape
    given = dict(vis=vis)
    if depth is not None:
        given["depth"] = depth = _lib.arg(depth, torch.float32, (None, H, W), who, "depth")
        given["frame"] = frame = _lib.arg(frame, torch.int32, (N,), who, "frame")
    else:
        frame = None
    cum = offsets = None
    if masks is not None:
        given["cum"], given["offsets"] = cum, offsets = mask_lists(who, masks, "None or ")
        given["det"] = det = _lib.arg(det, torch.int32, (N,), who, "det")
    else:
        det = None
    given["box"] = box = _lib.arg(box, torch.int32, (N, 4), who, "box")
    given["tol"] = tol = _lib.arg(tol, torch.float64, (N,), who, "tol")
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: HypothesisVerifier chunks)")
    if H < 1 or W < 1 or H * W > MAX_PIXELS or (depth is not None and depth.shape[0] < 1):
        raise ValueError(f"{who}: bad sizes (H, W > 0, H*W <= 2^22, M >= 1)")
    _lib.on_gpu(who, **given)
    if out is None:
        out = torch.empty(N, COUNTS, dtype=torch.int64, device=vis.device), torch.empty(N, dtype=torch.int32, device=vis.device)
    rows = _lib.arg(out[0], torch.int64, (N, COUNTS), who, "counts")
    status = _lib.arg(out[1], torch.int32, (N,), who, "status")
    _lib.on_gpu(who, counts=rows, status=status)
    _call("gpv_counts", vis, depth, 0 if depth is None else depth.shape[0], frame, cum, offsets, 0 if cum is None else cum.shape[0],
          0 if cum is None else offsets.shape[0] - 1, det, box, tol, N, H, W, rows, status, _lib.stream_ptr())
    return rows, status


# ------------------------------------------------------------------------------------------------ csv
def read_hypotheses(path):
    """evaluate.read_estimates plus "instance_id": the csv's column where it has one (`...MultiHypothesis.csv`), else the row
    number, so that every row of a top-1 file is an instance of its own."""
    import pandas as pd

    out = read_estimates(path)
    table = pd.read_csv(path, usecols=lambda c: c == "instance_id")
    ids = table["instance_id"].tolist() if "instance_id" in table.columns else range(len(out))
    for e, i in zip(out, ids):
        e["instance_id"] = int(i)
    return out


# ------------------------------------------------------------------------------------------------ the scores (host)
def verification_scores(counts, mask_area=None, status=None, clipped=None, min_points=32, occlusion_weight=0.0, tol=1.0, depth=True):
    """Rows of counts (N,16) on the host -> {"verify", "depth_fit", "iou", "residual"}, float64 (N,).  With c0 .. c9 a row:
        agree = c2 + c3      behind = c4 + c5      covered = c0 + .. + c7      inter = c1 + c3 + c5 + c7
        front = c7 + occlusion_weight * c6   for a pair with a mask: what lies in front of the drawn surface OUTSIDE the mask is an
                occluder the detector did not take for the object, and counts with `occlusion_weight` only;
              = c6 + c7                      for a pair without one (every pixel counts as inside)
        depth_fit = agree / ((agree + behind) + front),  0 when agree < min_points
        iou       = inter / ((covered + mask_area) - inter),  0 when the denominator is 0 or the pair has no mask
        verify    = depth_fit * iou with depth and a mask;  depth_fit with depth only;  iou with a mask only (depth=False);
                    0 where covered == 0, where a status bit is set, or where the view was clipped
        residual  = ((tol * c9) * 2^-20) / agree: the mean |measured - drawn| over the agreeing pixels, NaN without any
    mask_area (N,): the area of the pair's mask over the WHOLE frame (the sum of the odd-numbered run lengths), NaN for a pair
    without a mask; None: no pair has one.  tol: a number or (N,), what gpv_counts was given."""
    c = np.asarray(counts, np.int64).reshape(-1, COUNTS)
    N = len(c)
    area = np.full(N, np.nan) if mask_area is None else np.asarray(mask_area, np.float64).reshape(N)
    has_mask = ~np.isnan(area)
    agree, behind = c[:, 2] + c[:, 3], c[:, 4] + c[:, 5]
    covered = c[:, :8].sum(axis=1)
    inter = c[:, 1] + c[:, 3] + c[:, 5] + c[:, 7]
    front = np.where(has_mask, c[:, 7] + float(occlusion_weight) * c[:, 6], (c[:, 6] + c[:, 7]).astype(np.float64))
    with np.errstate(all="ignore"):
        den = (agree + behind) + front
        depth_fit = np.where((agree < min_points) | (den == 0), 0.0, agree / den)
        union = (covered + area) - inter
        iou = np.where(has_mask & (union != 0), inter / union, 0.0)
        verify = np.where(has_mask, depth_fit * iou, depth_fit) if depth else iou
        dead = covered == 0
        if status is not None:
            dead = dead | (np.asarray(status).reshape(N) != 0)
        if clipped is not None:
            dead = dead | (np.asarray(clipped).reshape(N) != 0)
        t = np.broadcast_to(np.asarray(tol, np.float64), (N,))
        residual = np.where(agree > 0, ((t * c[:, RESIDUAL]) * 2.0 ** -QUANTUM_BITS) / agree, np.nan)
    return dict(verify=np.where(dead, 0.0, verify), depth_fit=depth_fit, iou=iou, residual=residual)


def _instance_key(e, i):
    return (int(e["scene_id"]), int(e["im_id"]), int(e["instance_id"]) if "instance_id" in e else ("row", i))


# ------------------------------------------------------------------------------------------------ the verifier
class HypothesisVerifier(HypothesisFlow):
    """Verification scores of pose hypotheses, and the choice among the hypotheses of each detection.
      models   {obj_id: {"vertices" (V,3), "faces" (F,3), "diameter"}}            (what DepthRefiner and PoseScorer take)
      cameras  {(scene_id, im_id): {"cam_K" 9, ["depth" (H,W) z-depth in the units of the models, 0 = no measurement], ["size" (H, W)]}}
               "depth" is given for every frame or for none: none is the RGB-only case, masks are then required and the frame
               size is "size" or that of the masks
      tol         x diameter: measured and drawn depth AGREE when |measured - drawn| <= tol
      min_points  fewer agreeing pixels give depth_fit 0      occlusion_weight  see verification_scores
      box         "projected": the projected model's bounding box padded by `margin` pixels, joined with the bounding box of the
                  pair's mask (iou counts the mask's pixels that the drawing misses); "frame": the whole frame
      pairs_per_call  chunk size; by default the key buffer of one call stays below render.VIS_BYTES_PER_CALL
    .score(estimates, masks) takes the dictionaries read_hypotheses returns and gives back copies with "verify", "depth_fit",
    "iou", "residual", "verify_status" (STATUS_BITS, | refine.CLIPPED for a view that drops a triangle) and "counts" (the row of
    16) added.  masks: {instance_id: segmentation} or one segmentation per estimate (None = none for it), a COCO dict {"size":
    [H, W], "counts": run lengths, or a compressed string (decoded on the host by rle_strings)} -- or a hypotheses.DeviceMasks,
    lists that are on the device already (gtinfo.GroundTruthInfo.compute makes them), named by "instance_id".  Per chunk: render.project ->
    render.raster -> counts; the host does not synchronise inside the loop and no depth map, key or mask crosses PCIe again."""

    def __init__(self, models, cameras, tol=0.05, min_points=32, occlusion_weight=0.0, box="projected", margin=8, znear=1e-3,
                 pairs_per_call=None, device="cuda"):
        who = "HypothesisVerifier"
        if not (tol >= 0):
            raise ValueError(f"{who}: tol must be >= 0")
        if int(min_points) != min_points or min_points < 0:
            raise ValueError(f"{who}: min_points must be an integer >= 0, got {min_points!r}")
        if not (0 <= occlusion_weight <= 1):
            raise ValueError(f"{who}: occlusion_weight must lie in [0, 1]")
        if box not in ("projected", "frame"):
            raise ValueError(f"{who}: box must be 'projected' or 'frame'")
        self.tol, self.min_points, self.occlusion_weight = float(tol), int(min_points), float(occlusion_weight)
        super().__init__(who, models, cameras, "all_or_none", box, margin, znear, pairs_per_call, device)

    @torch.no_grad()
    def score(self, estimates, masks=None):
        who = "HypothesisVerifier.score"
        estimates = list(estimates)
        E = len(estimates)
        has_depth = self.table.depth_host is not None
        if masks is None and not has_depth:
            raise ValueError(f"{who}: no camera has a depth image: masks are required")
        groups = self._groups(who, estimates)
        on_device = isinstance(masks, DeviceMasks)
        lists = None if masks is None or on_device else pack_masks(who, estimates, masks, self.table)
        need_gpu(who, self.device)
        dev, depth = self.device, self.table.depth_on(self.device)
        area, cum_d, det_h, mask_boxes = np.full(E, np.nan), None, None, None
        if on_device and len(masks.areas):
            det_h, area, mask_boxes = masks.assign(who, estimates, self.table)
            cum_d = masks.lists
        elif lists is not None and len(lists[0]):
            runs, offsets, det_h, area, mask_boxes = lists
            cum_d = scan_masks(runs, offsets, self.H, self.W, dev)
        results = []                                   # (indices, counts, status, clipped, tol) on the device: read once at the end
        for ch in self._chunks(who, estimates, groups, det=det_h, mask_boxes=mask_boxes):      # the mask's box joins unpadded
            nb, t = len(ch.idx), self.tol * float(ch.model["diameter"])
            poses32 = torch.from_numpy(ch.poses.astype(np.float32)).to(dev)
            tol = torch.full((nb,), t, dtype=torch.float64, device=dev)
            clipped = torch.empty(nb, dtype=torch.int32, device=dev)
            rows, status = counts(ch.draw(poses32, clipped), depth, ch.frame, cum_d, ch.det, ch.box, tol)
            results.append((ch.idx, rows, status, clipped, t))
        out = [dict(e) for e in estimates]
        for idx, rows, status, clipped, t in results:
            rows, status, clipped = (x.cpu().numpy() for x in (rows, status, clipped))
            s = verification_scores(rows, area[idx] if cum_d is not None else None, status, clipped, self.min_points, self.occlusion_weight, t,
                                    has_depth)
            for j, i in enumerate(idx):
                out[i].update(verify=float(s["verify"][j]), depth_fit=float(s["depth_fit"][j]), iou=float(s["iou"][j]),
                              residual=float(s["residual"][j]), verify_status=int(status[j]) | (refine.CLIPPED if clipped[j] else 0),
                              counts=rows[j].copy())
        return out

    def _ranked(self, estimates, masks, score):
        if score not in ("coarse", "verify"):
            raise ValueError("HypothesisVerifier: score must be 'coarse' or 'verify'")
        scored = self.score(estimates, masks)
        by_instance = {}
        for i, e in enumerate(scored):
            by_instance.setdefault(_instance_key(e, i), []).append((-e["verify"], -float(e["score"]), i))
        groups = [[scored[i] for _, _, i in sorted(members)] for members in by_instance.values()]
        if score == "verify":
            for e in scored:
                e["coarse_score"], e["score"] = e["score"], e["verify"]
        return groups

    def rank(self, estimates, masks=None, score="coarse"):
        """The scored estimates with the hypotheses of each (scene_id, im_id, instance_id) together and best first: the largest
        "verify", a tie to the larger coarse "score", then to the earlier position; instances in the order of first appearance (an
        estimate without an instance_id is an instance of its own).  score="verify" writes the verification score into "score"
        (the coarse one is kept as "coarse_score")."""
        return [e for group in self._ranked(estimates, masks, score) for e in group]

    def select(self, estimates, masks=None, score="coarse"):
        """rank(), keeping the first of every instance: one estimate per detection, what refine.write_estimates and
        PoseScorer.score take."""
        return [group[0] for group in self._ranked(estimates, masks, score)]


def refine_and_select(refiner, verifier, estimates, masks=None, score="coarse"):
    """The flow of the reference's multi-hypothesis refiners: refine every hypothesis (refiner.refine: an estimate with a
    refine.STOP bit comes back with its input pose and takes part with it), then keep per detection the one that fits best
    (verifier.select)."""
    return verifier.select(refiner.refine(list(estimates)), masks, score)
