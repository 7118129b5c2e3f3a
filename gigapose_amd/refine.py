"""Refining pose estimates against the sensor's depth ON the GPU: point-to-plane ICP with same-pixel association
(libgigapose_refine.so, C-ABI: include/gigapose_refine.h, which spells the arithmetic out; gigapose_testing/refine_ref.py
restates it in numpy and tests/test_gpu_refine.py holds the kernels to it bit for bit).  The reference hands GigaPose's coarse
pose to a refiner; its RGB-D one (src/megapose/inference/icp_refiner.py) renders depth with Panda3D and calls
cv2.ppf_match_3d_ICP, neither of which an Instinct accelerator has.  This module takes that refiner's role with the parts the
project has: the estimate is drawn by the compute rasteriser (render.project + render.raster: a z-buffer of 64-bit keys), every
covered pixel whose measured depth lies within a gate of the drawn one adds a row to the Gauss-Newton normal equations of a
small rigid motion (gpf_accumulate: integer sums of quantised terms, so their bits depend on no summation order), and the
motion that solves them (unpivoted LDL^T, Cayley transform: no root, no transcendental) is applied (gpf_update).

  face_normals(vertices, faces)                 -> c f64 (F,3), unnormalised, once per mesh
  accumulate(vis, c, poses, K, depth, frame, box, gate, scale)   -> sums int64 (N,32), status int32 (N,)
  update(sums, clipped, scale, start, poses, poses32, state, ...) the step, in place
  DepthRefiner(models, cameras, ...)            .refine(estimates) -> a copy with R, t replaced + status, inliers, covered, rms
  write_estimates(path, estimates)              the csv evaluate.read_estimates reads: csv -> refine -> csv -> PoseScorer.score_csv
Out of scope: nearest-neighbour association (a point is compared with the measurement on its own ray), robust kernels beyond
the gate, the MegaPose network, colour; scores are left as they are (choosing among hypotheses: gigapose_amd/verify.py).  There is no CPU fallback: a
missing library is an error.
"""
import math

import numpy as np
import torch

from . import _lib
from .hypotheses import MAX_PAIRS_PER_CALL, MAX_PIXELS, HypothesisFlow, need_gpu, pose_matrix, projected_boxes  # noqa: F401  (gigapose_refine.h: Limits)

SUMS, SUM_RHS, SUM_EE, SUM_COVERED, SUM_COUNT = 32, 21, 27, 28, 29
QUANTUM_BITS = 36
RANGE, BAD_INDEX, FEW, DEGENERATE, CLIPPED, CONVERGED = 1, 2, 4, 8, 16, 32
STOP = FEW | DEGENERATE | CLIPPED
STATUS_BITS = {RANGE: "a pixel was dropped: a term left the range", BAD_INDEX: "a key names a face outside the mesh or a face without a finite normal",
               FEW: "fewer associated pixels than min_points", DEGENERATE: "a pivot of the normal equations is not above min_pivot x count",
               CLIPPED: "the view drops a triangle", CONVERGED: "the last step was below tol"}
_refine = _lib.SideLibrary("libgigapose_refine.so", "gpf")
REFINE_LIB_PATH, lib, _call = _refine.path, _refine.lib, _refine.call


def pixels_per_workgroup():
    return int(lib().gpf_pixels_per_workgroup())


@torch.no_grad()
def face_normals(vertices, faces):
    """gpf_face_normals: vertices f32 (V,3), faces int32 (F,3) on the device -> c f64 (F,3): (v1-v0) x (v2-v0), not normalised;
    NaN for a face with a vertex index outside [0, V)."""
    who = "face_normals"
    vertices = _lib.arg(vertices, torch.float32, (None, 3), who, "vertices")
    faces = _lib.arg(faces, torch.int32, (None, 3), who, "faces")
    if vertices.shape[0] < 1:
        raise ValueError(f"{who}: V = 0 vertices")
    _lib.on_gpu(who, vertices=vertices, faces=faces)
    c = torch.empty(faces.shape[0], 3, dtype=torch.float64, device=vertices.device)
    _call("gpf_face_normals", vertices, vertices.shape[0], faces, faces.shape[0], c, _lib.stream_ptr())
    return c


@torch.no_grad()
def accumulate(vis, c, poses, K, depth, frame, box, gate, scale, out=None):
    """gpf_accumulate: vis int64 (N,H,W) holding render.raster's keys, c f64 (F,3), poses f64 (N,4,4), K f64 (N,9), depth f32
    (M,H,W), frame int32 (N,), box int32 (N,4) x0 y0 x1 y1 inclusive, gate, scale f64 (N,), all on the device -> sums int64
    (N,32), status int32 (N,) on the device.  N <= 65535, H*W <= 2^22.  `out` = (sums, status) are buffers to write into."""
    who = "accumulate"
    vis = _lib.arg(vis, torch.int64, (None, None, None), who, "vis")
    N, H, W = vis.shape
    c = _lib.arg(c, torch.float64, (None, 3), who, "c")
    poses = _lib.arg(poses, torch.float64, (N, 4, 4), who, "poses")
    K = _lib.arg(K, torch.float64, (N, 9), who, "K")
    depth = _lib.arg(depth, torch.float32, (None, H, W), who, "depth")
    frame = _lib.arg(frame, torch.int32, (N,), who, "frame")
    box = _lib.arg(box, torch.int32, (N, 4), who, "box")
    gate = _lib.arg(gate, torch.float64, (N,), who, "gate")
    scale = _lib.arg(scale, torch.float64, (N,), who, "scale")
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: DepthRefiner chunks)")
    if H < 1 or W < 1 or H * W > MAX_PIXELS or depth.shape[0] < 1:
        raise ValueError(f"{who}: bad sizes (H, W > 0, H*W <= 2^22, M >= 1)")
    _lib.on_gpu(who, vis=vis, c=c, poses=poses, K=K, depth=depth, frame=frame, box=box, gate=gate, scale=scale)
    if out is None:
        out = torch.empty(N, SUMS, dtype=torch.int64, device=vis.device), torch.empty(N, dtype=torch.int32, device=vis.device)
    sums = _lib.arg(out[0], torch.int64, (N, SUMS), who, "sums")
    status = _lib.arg(out[1], torch.int32, (N,), who, "status")
    _lib.on_gpu(who, sums=sums, status=status)
    _call("gpf_accumulate", vis, c, c.shape[0], poses, K, depth, depth.shape[0], frame, box, gate, scale, N, H, W, sums, status, _lib.stream_ptr())
    return sums, status


def _check_step(who, min_points, min_pivot, damping, tol2):
    if int(min_points) != min_points or min_points < 0:
        raise ValueError(f"{who}: min_points must be an integer >= 0, got {min_points!r}")
    for what, v in (("min_pivot", min_pivot), ("damping", damping)):
        if not (v >= 0 and math.isfinite(v)):
            raise ValueError(f"{who}: {what} must be finite and >= 0, got {v!r}")
    if not tol2 >= 0:
        raise ValueError(f"{who}: tol2 must be >= 0, got {tol2!r}")


@torch.no_grad()
def update(sums, clipped, scale, start, poses, poses32, state, min_points=32, min_pivot=1e-3, damping=0.0, tol2=1e-12):
    """gpf_update: sums int64 (N,32), clipped int32 (N,) or None, scale f64 (N,), start f64 (N,4,4) or None; IN PLACE: poses f64
    (N,4,4), poses32 f32 (N,4,4), state int32 (N,).  A pair whose state holds a STOP bit is not touched; a pair that stops now gets
    `start` back where it is given."""
    who = "update"
    sums = _lib.arg(sums, torch.int64, (None, SUMS), who, "sums")
    N = sums.shape[0]
    clipped = None if clipped is None else _lib.arg(clipped, torch.int32, (N,), who, "clipped")
    scale = _lib.arg(scale, torch.float64, (N,), who, "scale")
    start = None if start is None else _lib.arg(start, torch.float64, (N, 4, 4), who, "start")
    poses = _lib.arg(poses, torch.float64, (N, 4, 4), who, "poses")
    poses32 = _lib.arg(poses32, torch.float32, (N, 4, 4), who, "poses32")
    state = _lib.arg(state, torch.int32, (N,), who, "state")
    _check_step(who, min_points, min_pivot, damping, tol2)
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: DepthRefiner chunks)")
    given = {k: v for k, v in dict(clipped=clipped, start=start).items() if v is not None}
    _lib.on_gpu(who, sums=sums, scale=scale, poses=poses, poses32=poses32, state=state, **given)
    _call("gpf_update", sums, clipped, scale, start, N, int(min_points), min_pivot, damping, tol2, poses, poses32, state, _lib.stream_ptr())
    return poses, poses32, state


# ------------------------------------------------------------------------------------------------ the statistics (host)
def rms_from_sums(sums, scale):
    """sums (N,32) int64 on the host, scale (N,) -> the root mean square point-to-plane distance of the associated pixels in
    model units, float64 (N,): scale * sqrt(sum 27 * 2^-36 / count), numpy's root; NaN where nothing is associated."""
    s = np.asarray(sums, np.int64)
    with np.errstate(all="ignore"):
        return np.asarray(scale, np.float64) * np.sqrt(s[:, SUM_EE].astype(np.float64) * 2.0 ** -QUANTUM_BITS / s[:, SUM_COUNT].astype(np.float64))


# ------------------------------------------------------------------------------------------------ the refiner
class DepthRefiner(HypothesisFlow):
    """Point-to-plane ICP of pose estimates against the sensor's depth.
      models   {obj_id: {"vertices" (V,3), "faces" (F,3), "diameter"}}            (what PoseScorer takes)
      cameras  {(scene_id, im_id): {"cam_K" 9, "depth" (H,W) z-depth in the units of the models, 0 = no measurement}}
      iters       Gauss-Newton iterations             gate       x diameter: a pixel is associated when |measured - drawn| <= gate
      min_points  fewer associated pixels stop a pair   min_pivot  x count: a pivot of the LDL^T not above it stops a pair
      damping     x count, added to the diagonal      tol        a step with |xi| below it is reported as converged
      box         "projected": the projected model's bounding box at the START pose padded by `margin` pixels; "frame": the whole
                  frame; or pass boxes=[(x0, y0, x1, y1) inclusive, ...] to refine(), one per estimate (the detection boxes)
      pairs_per_call  chunk size; by default the key buffer of one call stays below render.VIS_BYTES_PER_CALL
    .refine(estimates) takes the dictionaries evaluate.read_estimates returns and gives back copies with "R", "t" replaced, and
      "status"   the bits of STATUS_BITS: the pair's state | the last accumulation's status
      "inliers"  associated pixels at the returned pose        "covered"  pixels of the box the returned pose draws
      "rms"      the root mean square point-to-plane distance over the inliers, in model units (NaN without inliers)
    An estimate with a STOP bit (FEW, DEGENERATE, CLIPPED) keeps its INPUT pose, as the reference does when its ICP fails; the
    statistics are then the input pose's.  Scores are left as they are.  Per chunk: iters x (render.project -> render.raster ->
    accumulate -> update) and one last project / raster / accumulate; the host does not synchronise inside the loop and no depth
    map or key crosses PCIe."""

    def __init__(self, models, cameras, iters=10, gate=0.25, min_points=32, min_pivot=1e-3, damping=0.0, tol=1e-6, box="projected",
                 margin=8, znear=1e-3, pairs_per_call=None, device="cuda"):
        who = "DepthRefiner"
        if int(iters) != iters or iters < 0:
            raise ValueError(f"{who}: iters must be an integer >= 0")
        if not (gate >= 0):
            raise ValueError(f"{who}: gate must be >= 0")
        if box not in ("projected", "frame"):
            raise ValueError(f"{who}: box must be 'projected' or 'frame'")
        _check_step(who, min_points, min_pivot, damping, tol * tol)
        self.iters, self.gate = int(iters), float(gate)
        self.step = dict(min_points=int(min_points), min_pivot=float(min_pivot), damping=float(damping), tol2=float(tol) * float(tol))
        super().__init__(who, models, cameras, "required", box, margin, znear, pairs_per_call, device)

    @torch.no_grad()
    def refine(self, estimates, boxes=None):
        who = "DepthRefiner.refine"
        estimates = list(estimates)
        E = len(estimates)
        if boxes is not None:
            boxes = np.asarray(boxes)
            if boxes.shape != (E, 4) or boxes.dtype.kind not in "iu":
                raise ValueError(f"{who}: expected boxes integers ({E}, 4), got {boxes.dtype} {boxes.shape}")
        groups = self._groups(who, estimates)
        need_gpu(who, self.device)
        dev, depth = self.device, self.table.depth_on(self.device)
        results = []                                   # (indices, poses, state, status, sums) on the device: read once at the end
        for ch in self._chunks(who, estimates, groups, boxes):
            if ch.first:
                c, d = face_normals(ch.vertices, ch.faces), float(ch.model["diameter"])
            nb = len(ch.idx)
            poses = torch.from_numpy(ch.poses).to(dev)
            start, poses32 = poses.clone(), poses.to(torch.float32)
            Kd = torch.from_numpy(ch.K).to(dev)
            gate = torch.full((nb,), self.gate * d, dtype=torch.float64, device=dev)
            scale = torch.full((nb,), d, dtype=torch.float64, device=dev)
            state = torch.zeros(nb, dtype=torch.int32, device=dev)
            clipped = torch.empty(nb, dtype=torch.int32, device=dev)
            out = torch.empty(nb, SUMS, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
            for it in range(self.iters + 1):
                sums, status = accumulate(ch.draw(poses32, clipped), c, poses, Kd, depth, ch.frame, ch.box, gate, scale, out=out)
                if it < self.iters:
                    update(sums, clipped, scale, start, poses, poses32, state, **self.step)
            results.append((ch.idx, poses, state, status, sums, clipped, d))
        out = [dict(e) for e in estimates]
        for idx, poses, state, status, sums, clipped, d in results:
            poses, state, status, sums, clipped = (t.cpu().numpy() for t in (poses, state, status, sums, clipped))
            rms = rms_from_sums(sums, np.full(len(idx), d))
            for j, i in enumerate(idx):
                bits = int(state[j]) | int(status[j]) | (CLIPPED if clipped[j] else 0)
                if bits & STOP and not int(state[j]) & STOP:     # the LAST view is the first that drops a triangle: the input pose
                    poses[j] = pose_matrix(estimates[i]["R"], estimates[i]["t"])
                out[i]["R"], out[i]["t"] = poses[j, :3, :3].copy(), poses[j, :3, 3].copy()
                out[i].update(status=bits, inliers=int(sums[j, SUM_COUNT]), covered=int(sums[j, SUM_COVERED]), rms=float(rms[j]))
        return out


def write_estimates(path, estimates):
    """The csv evaluate.read_estimates reads (the columns inout.save_predictions_from_batched_predictions writes: scene_id, im_id,
    obj_id, score, R, t, time), one row per estimate in order; "time" is carried where an estimate has it, else -1.  Floats are
    written with their shortest round-trip text: read_estimates gives back scene_id, im_id, obj_id, score, R and t to the bit."""
    def floats(a):
        return " ".join(map(str, np.asarray(a, np.float64).flatten().tolist()))

    lines = ["scene_id,im_id,obj_id,score,R,t,time"]
    for e in estimates:
        R, t = np.asarray(e["R"], np.float64), np.asarray(e["t"], np.float64)
        if R.size != 9 or t.size != 3:
            raise ValueError("write_estimates: an estimate's R / t does not hold 9 / 3 numbers")
        lines.append("{},{},{},{},{},{},{}".format(int(e["scene_id"]), int(e["im_id"]), int(e["obj_id"]), float(e["score"]), floats(R), floats(t),
                                                   e.get("time", -1)))
    with open(path, "w") as fh:
        fh.write("\n".join(lines))
    return path
