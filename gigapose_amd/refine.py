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
import ctypes
import math

import numpy as np
import torch

from . import _lib, render
from .evaluate import pose_matrix

MAX_PAIRS_PER_CALL = 65535                           # the grid's second dimension (gigapose_refine.h: Limits)
MAX_PIXELS = 1 << 22                                 # H*W: the bound on an integer sum
SUMS, SUM_RHS, SUM_EE, SUM_COVERED, SUM_COUNT = 32, 21, 27, 28, 29
QUANTUM_BITS = 36
RANGE, BAD_INDEX, FEW, DEGENERATE, CLIPPED, CONVERGED = 1, 2, 4, 8, 16, 32
STOP = FEW | DEGENERATE | CLIPPED
STATUS_BITS = {RANGE: "a pixel was dropped: a term left the range", BAD_INDEX: "a key names a face outside the mesh or a face without a finite normal",
               FEW: "fewer associated pixels than min_points", DEGENERATE: "a pivot of the normal equations is not above min_pivot x count",
               CLIPPED: "the view drops a triangle", CONVERGED: "the last step was below tol"}
_refine = _lib.SideLibrary("libgigapose_refine.so", "gpf")
REFINE_LIB_PATH, lib, _call = _refine.path, _refine.lib, _refine.call


def _d(v):
    return ctypes.c_double(float(v))


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
    _call("gpf_face_normals", _lib.ptr(vertices), _lib.i(vertices.shape[0]), _lib.ptr(faces), _lib.i(faces.shape[0]), _lib.ptr(c),
          _lib.stream_ptr())
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
    _call("gpf_accumulate", _lib.ptr(vis), _lib.ptr(c), _lib.i(c.shape[0]), _lib.ptr(poses), _lib.ptr(K), _lib.ptr(depth), _lib.i(depth.shape[0]),
          _lib.ptr(frame), _lib.ptr(box), _lib.ptr(gate), _lib.ptr(scale), _lib.i(N), _lib.i(H), _lib.i(W), _lib.ptr(sums), _lib.ptr(status),
          _lib.stream_ptr())
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
    _call("gpf_update", _lib.ptr(sums), _lib.ptr(clipped), _lib.ptr(scale), _lib.ptr(start), _lib.i(N), ctypes.c_longlong(int(min_points)),
          _d(min_pivot), _d(damping), _d(tol2), _lib.ptr(poses), _lib.ptr(poses32), _lib.ptr(state), _lib.stream_ptr())
    return poses, poses32, state


# ------------------------------------------------------------------------------------------------ boxes (host)
def projected_boxes(vertices, poses, K, H, W, margin):
    """The bounding box of the model's projected vertices at each pose, padded by `margin` pixels: float64 on the host, floor /
    ceil, clamped to [-1, W] x [-1, H] (the kernel clamps to the frame).  A pose that puts a vertex at z <= 0 or gives a value
    that is not finite takes the whole frame.  vertices (V,3), poses (N,4,4), K (N,9) -> int32 (N,4)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    out = np.zeros((len(poses), 4), np.int32)
    for n, (P, k) in enumerate(zip(np.asarray(poses, np.float64), np.asarray(K, np.float64).reshape(-1, 9))):
        p = v @ P[:3, :3].T + P[:3, 3]
        with np.errstate(all="ignore"):
            u = (k[0] * p[:, 0] + k[1] * p[:, 1]) / p[:, 2] + k[2]
            w = (k[4] * p[:, 1]) / p[:, 2] + k[5]
        if not (np.isfinite(u).all() and np.isfinite(w).all() and (p[:, 2] > 0).all()):
            out[n] = (0, 0, W - 1, H - 1)
            continue
        lo = np.clip(np.floor([u.min() - margin, w.min() - margin]), -1, [W, H])
        hi = np.clip(np.ceil([u.max() + margin, w.max() + margin]), -1, [W, H])
        out[n] = (lo[0], lo[1], hi[0], hi[1])
    return out


def rms_from_sums(sums, scale):
    """sums (N,32) int64 on the host, scale (N,) -> the root mean square point-to-plane distance of the associated pixels in
    model units, float64 (N,): scale * sqrt(sum 27 * 2^-36 / count), numpy's root; NaN where nothing is associated."""
    s = np.asarray(sums, np.int64)
    with np.errstate(all="ignore"):
        return np.asarray(scale, np.float64) * np.sqrt(s[:, SUM_EE].astype(np.float64) * 2.0 ** -QUANTUM_BITS / s[:, SUM_COUNT].astype(np.float64))


# ------------------------------------------------------------------------------------------------ the refiner
class DepthRefiner:
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
        self.models, self.device = models, device
        self.iters, self.gate, self.box, self.margin, self.znear = int(iters), float(gate), box, float(margin), float(znear)
        self.step = dict(min_points=int(min_points), min_pivot=float(min_pivot), damping=float(damping), tol2=float(tol) * float(tol))
        self.frames = sorted(cameras)
        if not self.frames:
            raise ValueError(f"{who}: no cameras")
        depth = [np.asarray(cameras[k]["depth"], np.float32) for k in self.frames]
        self.H, self.W = depth[0].shape
        if any(d.shape != (self.H, self.W) for d in depth):
            raise ValueError(f"{who}: the depth images differ in size")
        if self.H * self.W > MAX_PIXELS:
            raise ValueError(f"{who}: {self.H} x {self.W} frames (at most 2^22 pixels)")
        self._depth_host, self._depth = np.stack(depth), None
        self.K = {k: np.asarray(cameras[k]["cam_K"], np.float64).reshape(9) for k in self.frames}
        self._frame_index = {k: i for i, k in enumerate(self.frames)}
        limit = max(1, render.VIS_BYTES_PER_CALL // (self.H * self.W * 8))
        self.pairs_per_call = max(1, min(int(limit if pairs_per_call is None else pairs_per_call), MAX_PAIRS_PER_CALL))
        for o, m in models.items():
            if m.get("diameter") is None or not float(m["diameter"]) > 0:
                raise ValueError(f"{who}: model {o} needs a positive diameter")

    @torch.no_grad()
    def refine(self, estimates, boxes=None):
        who = "DepthRefiner.refine"
        estimates = list(estimates)
        E = len(estimates)
        if boxes is not None:
            boxes = np.asarray(boxes)
            if boxes.shape != (E, 4) or boxes.dtype.kind not in "iu":
                raise ValueError(f"{who}: expected boxes integers ({E}, 4), got {boxes.dtype} {boxes.shape}")
        groups = {}
        for i, e in enumerate(estimates):
            key, obj = (int(e["scene_id"]), int(e["im_id"])), int(e["obj_id"])
            if key not in self._frame_index:
                raise ValueError(f"{who}: estimate {i}: image {key} has no camera")
            if obj not in self.models:
                raise ValueError(f"{who}: estimate {i}: object {obj} has no model")
            groups.setdefault((obj, self.K[key].tobytes()), []).append(i)
        if torch.device(self.device).type != "cuda":
            raise _lib.GigaPoseHipError(f"{who} needs a GPU device (no CPU fallback)")
        if self._depth is None:
            self._depth = torch.from_numpy(self._depth_host).to(self.device)
        dev, H, W = self.device, self.H, self.W
        results = []                                   # (indices, poses, state, status, sums) on the device: read once at the end
        for (obj, _), idx in sorted(groups.items(), key=lambda kv: kv[1][0]):
            m = self.models[obj]
            vertices, faces = _lib.upload(who, dev, _lib.checked(m["vertices"], torch.float32, (None, 3), who, "vertices"),
                                          _lib.checked(m["faces"], torch.int32, (None, 3), who, "faces"))
            c = face_normals(vertices, faces)
            d = float(m["diameter"])
            poses_h = np.stack([pose_matrix(estimates[i]["R"], estimates[i]["t"]) for i in idx])
            keys = [(int(estimates[i]["scene_id"]), int(estimates[i]["im_id"])) for i in idx]
            K_h = np.stack([self.K[k] for k in keys])
            if boxes is not None:
                box_h = np.ascontiguousarray(boxes[idx], np.int32)
            elif self.box == "frame":
                box_h = np.tile(np.asarray([0, 0, W - 1, H - 1], np.int32), (len(idx), 1))
            else:
                box_h = projected_boxes(m["vertices"], poses_h, K_h, H, W, self.margin)
            K9 = render._k9(K_h[0])
            V, F = vertices.shape[0], faces.shape[0]
            n = min(len(idx), self.pairs_per_call)
            xy = torch.empty(n, V, 2, dtype=torch.int32, device=dev)
            vdepth = torch.empty(n, V, dtype=torch.float32, device=dev)
            vis = torch.empty(n, H, W, dtype=torch.int64, device=dev)
            work = torch.empty(max(1, -(-int(render.lib().gpr_raster_workspace_bytes(_lib.i(n), _lib.i(F))) // 8)), dtype=torch.int64, device=dev)
            for _, a, b in _lib.chunked(len(idx), self.pairs_per_call):
                nb = b - a
                poses = torch.from_numpy(poses_h[a:b]).to(dev)
                start, poses32 = poses.clone(), poses.to(torch.float32)
                Kd = torch.from_numpy(np.ascontiguousarray(K_h[a:b])).to(dev)
                frame = torch.tensor([self._frame_index[k] for k in keys[a:b]], dtype=torch.int32, device=dev)
                box = torch.from_numpy(np.ascontiguousarray(box_h[a:b])).to(dev)
                gate = torch.full((nb,), self.gate * d, dtype=torch.float64, device=dev)
                scale = torch.full((nb,), d, dtype=torch.float64, device=dev)
                state = torch.zeros(nb, dtype=torch.int32, device=dev)
                clipped = torch.empty(nb, dtype=torch.int32, device=dev)
                out = torch.empty(nb, SUMS, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
                for it in range(self.iters + 1):
                    pxy, pz = render.project(vertices, poses32, K9, self.znear, out=(xy, vdepth))
                    keys_d, _ = render.raster(pxy, pz, faces, H, W, out=(vis, clipped), workspace=work)
                    sums, status = accumulate(keys_d, c, poses, Kd, self._depth, frame, box, gate, scale, out=out)
                    if it < self.iters:
                        update(sums, clipped, scale, start, poses, poses32, state, **self.step)
                results.append((idx[a:b], poses, state, status, sums, clipped, d))
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
