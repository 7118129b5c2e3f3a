"""Fitting coarse poses to the detection's mask ON the GPU: the silhouette's moments (libgigapose_maskfit.so, C-ABI:
include/gigapose_maskfit.h, which spells the arithmetic out; gigapose_testing/maskfit_ref.py restates it and
tests/test_gpu_maskfit.py holds the kernels to it bit for bit).  GigaPose is an RGB method and its coarse stage regresses four
degrees of freedom per correspondence -- the in-plane angle, the scale (so t_z) and the 2-D translation; the detection's mask,
already on the device as the ingest library's prefix sums, is direct evidence for exactly those four.  The pose is drawn by the
compute rasteriser (render.project + render.raster: a z-buffer of 64-bit keys), gpm_moments sums the moments of order 0, 1 and 2
of its covered pixels with its intersection with the mask, gpm_mask_moments sums the mask's moments in closed form from its
runs, and gpm_update turns, scales and shifts the pose so that the two sets of moments meet (a rational rule: no root, no
transcendental), keeping the pose of the best intersection over union.  Integer sums: their bits depend on no summation order.

  mask_moments(masks, H, W)                        -> mm int64 (D,8), mstatus int32 (D,)
  moments(vis, masks, det, box)                    -> rows int64 (N,16), status int32 (N,)
  update(rows, status, mm, det, clipped, K, start, it, last, poses, poses32, best, score, state, ...)   the step, in place
  MaskRefiner(models, cameras, ...)                .refine(estimates, masks) -> copies with R, t replaced + maskfit_status, iou ...
  fit_refine_and_select(fitter, refiner, verifier, estimates, masks)   fit -> refiner.refine -> verifier.select
Out of scope: occlusion (the mask of a half-hidden object pulls the fit towards the visible part), the 180-degree ambiguity of
second moments (turns beyond 45 degrees are not attempted), out-of-plane rotation, cameras whose fx and fy differ much or with
skew, polygon masks.  There is no CPU fallback: a missing library is an error.
"""
import math

import numpy as np
import torch

from . import _lib
from .hypotheses import MAX_PAIRS_PER_CALL, MAX_PIXELS, HypothesisFlow, mask_lists, need_gpu, pack_masks, scan_masks  # (gigapose_maskfit.h: Limits)

MAX_SIDE = 16384                                     # H, W: a sum of x*x stays below 2^50
ROW, MASK_ROW, INTER, EDGE = 16, 8, 6, 7
BAD_MASK, NO_MASK, FEW, CLIPPED, ROUND, NOT_IMPROVED = 1, 2, 4, 8, 16, 32
STOP = BAD_MASK | NO_MASK | FEW | CLIPPED
STATUS_BITS = {BAD_MASK: "the detection index or its run-length list is bad", NO_MASK: "the estimate has no mask",
               FEW: "the drawing or the mask has fewer pixels than min_points", CLIPPED: "the view drops a triangle",
               ROUND: "the last step took no turn: a silhouette is too round, or the orientations are more than 45 degrees apart",
               NOT_IMPROVED: "the best pose is the input pose"}
_maskfit = _lib.SideLibrary("libgigapose_maskfit.so", "gpm")
MASKFIT_LIB_PATH, lib, _call = _maskfit.path, _maskfit.lib, _maskfit.call


def pixels_per_workgroup():
    return int(lib().gpm_pixels_per_workgroup())


def _frame(who, H, W):
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or H * W > MAX_PIXELS:
        raise ValueError(f"{who}: {H} x {W} frames (H, W in 1 .. 16384, H*W <= 2^22)")


@torch.no_grad()
def mask_moments(masks, H, W):
    """gpm_mask_moments: masks = (cum, offsets), int32 (total,) and (D+1,) on the device as ingest.RleDetectionPreprocessor.scan
    returns them -> mm int64 (D,8): n, sum x, y, xx, xy, yy of each mask, mstatus int32 (D,): BAD_MASK for a bad list."""
    who = "mask_moments"
    cum, offsets = mask_lists(who, masks)
    _frame(who, int(H), int(W))
    _lib.on_gpu(who, cum=cum, offsets=offsets)
    D = offsets.shape[0] - 1
    mm = torch.empty(D, MASK_ROW, dtype=torch.int64, device=cum.device)
    mstatus = torch.empty(D, dtype=torch.int32, device=cum.device)
    _call("gpm_mask_moments", cum, offsets, cum.shape[0], D, H, W, mm, mstatus, _lib.stream_ptr())
    return mm, mstatus


@torch.no_grad()
def moments(vis, masks, det, box, out=None):
    """gpm_moments: vis int64 (N,H,W) holding render.raster's keys; masks = (cum, offsets); det int32 (N,) into D, negative = no
    mask (NO_MASK); box int32 (N,4) x0 y0 x1 y1 inclusive, all on the device -> rows int64 (N,16), status int32 (N,) on the
    device.  N <= 65535, H*W <= 2^22, H, W <= 16384.  `out` = (rows, status) are buffers to write into."""
    who = "moments"
    vis = _lib.arg(vis, torch.int64, (None, None, None), who, "vis")
    N, H, W = vis.shape
    cum, offsets = mask_lists(who, masks)
    det = _lib.arg(det, torch.int32, (N,), who, "det")
    box = _lib.arg(box, torch.int32, (N, 4), who, "box")
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: MaskRefiner chunks)")
    _frame(who, H, W)
    _lib.on_gpu(who, vis=vis, cum=cum, offsets=offsets, det=det, box=box)
    if out is None:
        out = torch.empty(N, ROW, dtype=torch.int64, device=vis.device), torch.empty(N, dtype=torch.int32, device=vis.device)
    rows = _lib.arg(out[0], torch.int64, (N, ROW), who, "rows")
    status = _lib.arg(out[1], torch.int32, (N,), who, "status")
    _lib.on_gpu(who, rows=rows, status=status)
    _call("gpm_moments", vis, cum, offsets, cum.shape[0], offsets.shape[0] - 1, det, box, N, H, W, rows, status, _lib.stream_ptr())
    return rows, status


def _check_step(who, min_points, min_elongation, gain):
    if int(min_points) != min_points or min_points < 1:
        raise ValueError(f"{who}: min_points must be an integer >= 1, got {min_points!r}")
    if not (min_elongation >= 0 and math.isfinite(min_elongation)):
        raise ValueError(f"{who}: min_elongation must be finite and >= 0, got {min_elongation!r}")
    if not 0 < gain <= 1:
        raise ValueError(f"{who}: gain must lie in (0, 1], got {gain!r}")


def new_state(N, device):
    """The buffers gpm_update keeps per pair: best f64 (N,4,4), score int64 (N,4), state int32 (N,2).  The call with it = 0
    initialises them."""
    return (torch.empty(N, 4, 4, dtype=torch.float64, device=device), torch.empty(N, 4, dtype=torch.int64, device=device),
            torch.empty(N, 2, dtype=torch.int32, device=device))


@torch.no_grad()
def update(rows, status, mm, det, clipped, K, start, it, last, poses, poses32, best, score, state, min_points=32, min_elongation=0.1, gain=1.0):
    """gpm_update: rows int64 (N,16) and status int32 (N,) from moments at the current poses, mm int64 (D,8) from mask_moments,
    det int32 (N,), clipped int32 (N,) or None, K f64 (N,9), start f64 (N,4,4); `it` the number of the call in the loop (0
    initialises best, score and state), `last` = judge only; IN PLACE: poses f64 (N,4,4), poses32 f32 (N,4,4), best f64 (N,4,4),
    score int64 (N,4) (intersection, union of the best pose and of the input pose), state int32 (N,2) (status bits, the iteration
    the best pose came from)."""
    who = "update"
    rows = _lib.arg(rows, torch.int64, (None, ROW), who, "rows")
    N = rows.shape[0]
    status = _lib.arg(status, torch.int32, (N,), who, "status")
    mm = _lib.arg(mm, torch.int64, (None, MASK_ROW), who, "mm")
    det = _lib.arg(det, torch.int32, (N,), who, "det")
    clipped = None if clipped is None else _lib.arg(clipped, torch.int32, (N,), who, "clipped")
    K = _lib.arg(K, torch.float64, (N, 9), who, "K")
    start = _lib.arg(start, torch.float64, (N, 4, 4), who, "start")
    poses = _lib.arg(poses, torch.float64, (N, 4, 4), who, "poses")
    poses32 = _lib.arg(poses32, torch.float32, (N, 4, 4), who, "poses32")
    best = _lib.arg(best, torch.float64, (N, 4, 4), who, "best")
    score = _lib.arg(score, torch.int64, (N, 4), who, "score")
    state = _lib.arg(state, torch.int32, (N, 2), who, "state")
    _check_step(who, min_points, min_elongation, gain)
    if int(it) != it or it < 0:
        raise ValueError(f"{who}: it must be an integer >= 0, got {it!r}")
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: MaskRefiner chunks)")
    given = {} if clipped is None else dict(clipped=clipped)
    _lib.on_gpu(who, rows=rows, status=status, mm=mm, det=det, K=K, start=start, poses=poses, poses32=poses32, best=best, score=score, state=state, **given)
    _call("gpm_update", rows, status, mm, mm.shape[0], det, clipped, K, start, N, it, 1 if last else 0, int(min_points), min_elongation, gain, poses, poses32,
          best, score, state, _lib.stream_ptr())
    return poses, poses32, best, score, state


# ------------------------------------------------------------------------------------------------ the fitter
class MaskRefiner(HypothesisFlow):
    """The silhouette fit of pose estimates to their detections' masks.
      models   {obj_id: {"vertices" (V,3), "faces" (F,3), "diameter"}}            (what HypothesisVerifier takes)
      cameras  {(scene_id, im_id): {"cam_K" 9, ["size" (H, W)]}}   no depth is needed; the frame size is "size" or the masks'
      iters           steps of the fit                min_points  a drawing or a mask with fewer pixels stops its pair
      min_elongation  no turn is taken where a set's (principal second moments' difference) / (their sum) is below it
      gain            in (0, 1]: the share of each correction that is applied
      box         "projected": the START pose's projected bounding box joined with the bounding box of the pair's mask, padded by
                  `margin` pixels; "frame": the whole frame.  A pose whose drawing touches an edge of its box that is not an
                  edge of the frame is never kept as the best.
      pairs_per_call  chunk size; by default the key buffer of one call stays below render.VIS_BYTES_PER_CALL
    .refine(estimates, masks) takes the dictionaries verify.read_hypotheses returns and the mask forms of HypothesisVerifier.score
    ({instance_id: segmentation} or one segmentation per estimate, None = none for it) and gives back copies with "R", "t"
    replaced by the pose of the best intersection over union among the start and the poses after each step, and
      "maskfit_status"   the bits of STATUS_BITS     "iou_start", "iou"  of the input and of the returned pose (0 where unknown)
      "best_iteration"   0 = the input pose          "moments"  the row of 16 of the last pose drawn
      "iou_counts"       the integers behind the two: intersection, union of the returned pose, intersection, union of the input pose
    An estimate with a STOP bit, or whose best pose is its start, carries NOT_IMPROVED and its input pose, bit for bit.  Scores
    are left as they are.  Per chunk: iters x (render.project -> render.raster -> moments -> update), then one last draw, moments
    and an update that only judges; the host does not synchronise inside the loop and no key or mask crosses PCIe again."""

    def __init__(self, models, cameras, iters=8, min_points=32, min_elongation=0.1, gain=1.0, box="projected", margin=16, znear=1e-3,
                 pairs_per_call=None, device="cuda"):
        who = "MaskRefiner"
        if int(iters) != iters or iters < 0:
            raise ValueError(f"{who}: iters must be an integer >= 0")
        if box not in ("projected", "frame"):
            raise ValueError(f"{who}: box must be 'projected' or 'frame'")
        _check_step(who, min_points, min_elongation, gain)
        self.iters = int(iters)
        self.step = dict(min_points=int(min_points), min_elongation=float(min_elongation), gain=float(gain))
        super().__init__(who, models, cameras, "ignored", box, margin, znear, pairs_per_call, device)

    @torch.no_grad()
    def refine(self, estimates, masks):
        who = "MaskRefiner.refine"
        estimates = list(estimates)
        if masks is None:
            raise ValueError(f"{who}: masks are required")
        groups = self._groups(who, estimates)
        runs, offsets, det_h, _, mask_boxes = pack_masks(who, estimates, masks, self.table)
        need_gpu(who, self.device)
        dev, H, W = self.device, self.H, self.W
        _frame(who, H, W)
        out = [dict(e) for e in estimates]
        if not len(runs):                              # no estimate has a mask
            for o in out:
                o.update(maskfit_status=NO_MASK | NOT_IMPROVED, iou_start=0.0, iou=0.0, best_iteration=0, moments=np.zeros(ROW, np.int64),
                         iou_counts=np.asarray([0, 1, 0, 1], np.int64))
            return out
        lists = scan_masks(runs, offsets, H, W, dev)
        mm, _ = mask_moments(lists, H, W)
        results = []                                   # (indices, poses, score, state, rows) on the device: read once at the end
        # the mask's box joins padded like the projected one
        for ch in self._chunks(who, estimates, groups, det=det_h, mask_boxes=mask_boxes, pad=math.ceil(self.margin)):
            nb = len(ch.idx)
            poses = torch.from_numpy(ch.poses).to(dev)
            start, poses32 = poses.clone(), poses.to(torch.float32)
            Kd = torch.from_numpy(ch.K).to(dev)
            best, score, state = new_state(nb, dev)
            clipped = torch.empty(nb, dtype=torch.int32, device=dev)
            buffers = torch.empty(nb, ROW, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
            for it in range(self.iters + 1):
                rows, status = moments(ch.draw(poses32, clipped), lists, ch.det, ch.box, out=buffers)
                update(rows, status, mm, ch.det, clipped, Kd, start, it, it == self.iters, poses, poses32, best, score, state, **self.step)
            results.append((ch.idx, poses, score, state, rows))
        for idx, poses, score, state, rows in results:
            poses, score, state, rows = (t.cpu().numpy() for t in (poses, score, state, rows))
            for j, i in enumerate(idx):
                out[i]["R"], out[i]["t"] = poses[j, :3, :3].copy(), poses[j, :3, 3].copy()
                out[i].update(maskfit_status=int(state[j, 0]), iou_start=float(score[j, 2]) / float(score[j, 3]), iou=float(score[j, 0]) / float(score[j, 1]),
                              best_iteration=int(state[j, 1]), moments=rows[j].copy(), iou_counts=score[j].copy())
        return out


def fit_refine_and_select(fitter, refiner, verifier, estimates, masks, score="coarse"):
    """The coarse stage's hypotheses -> fitter.refine (the silhouette fit: an estimate that is stopped or not improved takes part
    with its input pose) -> refiner.refine (a refine.DepthRefiner; None on an RGB-only run) -> verifier.select: one estimate per
    detection."""
    fitted = fitter.refine(list(estimates), masks)
    if refiner is not None:
        fitted = refiner.refine(fitted)
    return verifier.select(fitted, masks, score)
