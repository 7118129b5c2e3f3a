"""Scoring pose estimates against ground truth ON the GPU: the BOP-19 errors MSSD, MSPD and VSD (Hodan et al., "BOP Challenge
2020", section 2.2) and the recall they give, for the csv files gigapose_amd/inout.py writes.  The reference shells out to
bop_toolkit's eval_bop19_pose.py with --renderer_type=vispy (src/scripts/eval_bop.py:29), which needs an OpenGL context; an
Instinct accelerator has none, so VSD's depth maps come from the compute rasteriser (render.MeshRenderer) and the errors from
libgigapose_eval.so (C-ABI: include/gigapose_eval.h, which spells the arithmetic out; gigapose_testing/eval_ref.py restates it in
numpy and tests/test_gpu_eval.py holds the kernels to it bit for bit).

  symmetry_transforms(model_info)        models_info.json entry -> (S,4,4) f64, the identity first
  mssd_mspd(...) / vsd_counts(...)       the two entry points on device tensors, <= 65535 pairs
  pose_errors(vertices, syms, est, gt, K)            -> mssd, mspd: torch f64 on the host (any number of pairs)
  vsd_errors(mesh, est, gt, K, depth_test, frame, diameter, ...)   renders both pose sets, -> {"errors", "counts", "clipped"}
  PoseScorer(models, targets, gts, cameras)          .score_csv(path) / .score(estimates) -> recalls, ar_mssd, ar_mspd, ar_vsd, ar
ADD, ADD-S and the model diameter are gigapose_amd/distances.py (libgigapose_dist.so: means over integers, so their bits do not
depend on the summation order).  The BOP-19 visibility filter of the ground truths is PoseScorer's min_visib over the "visib_fract" gigapose_amd/gtinfo.py computes.
Out of scope: reading BOP json and depth PNG files (PoseScorer is handed their contents), the bop18 visibility mode, near-plane clipping (an estimate that puts a vertex
behind the camera drops triangles: it is reported and scores VSD 1).  There is no CPU fallback: a missing library is an error.
"""
import math

import numpy as np
import torch

from . import _lib
from .hypotheses import CameraTable, pose_matrix  # noqa: F401  (pose_matrix is read from here too)
from .render import MeshRenderer

MAX_PAIRS_PER_CALL = 65535                           # the grid's second dimension (gigapose_eval.h: Limits)
MAX_THRESHOLDS = 16                                  # GPE_MAX_THRESHOLDS
WORKSPACE_BYTES_PER_CALL = 1 << 30                   # pose_errors: the (pair, symmetry) workspace of one call stays below this
DEPTH_BYTES_PER_CALL = 1 << 28                       # vsd_errors: each of the two depth stacks of one call stays below this
TAUS = tuple(round(0.05 * i, 2) for i in range(1, 11))           # VSD misalignment tolerances, x diameter
CORRECT_THS = tuple(round(0.05 * i, 2) for i in range(1, 11))    # thresholds of correctness: x diameter (MSSD), on e (VSD)
MSPD_THS = tuple(float(5 * i) for i in range(1, 11))             # px at W = 640
_eval = _lib.SideLibrary("libgigapose_eval.so", "gpe")
EVAL_LIB_PATH, lib, _call = _eval.path, _eval.lib, _eval.call


# ------------------------------------------------------------------------------------------------ symmetries
def _axis_rotation(axis, angle):
    a = np.asarray(axis, np.float64).reshape(3)
    norm = float(np.sqrt((a * a).sum()))
    if not norm > 0:
        raise ValueError("symmetry_transforms: a continuous symmetry has a zero axis")
    a = a / norm
    c, s = math.cos(angle), math.sin(angle)
    cross = np.asarray([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return c * np.eye(3) + s * cross + (1.0 - c) * np.outer(a, a)


def symmetry_transforms(model_info, max_sym_disc_step=0.01):
    """A models_info.json entry -> (S,4,4) float64, the identity first.  `symmetries_discrete`: 16 numbers each, row-major;
    `symmetries_continuous`: {"axis", "offset"} each, discretised into ceil(pi / max_sym_disc_step) rotations (315) about the
    axis through the offset.  Every discrete (the identity included) x continuous combination: R = Rc Rd, t = Rc td + tc."""
    if not max_sym_disc_step > 0:
        raise ValueError("symmetry_transforms: max_sym_disc_step must be positive")
    disc = [np.eye(4)]
    for m in model_info.get("symmetries_discrete", ()) or ():
        m = np.asarray(m, np.float64)
        if m.size != 16:
            raise ValueError("symmetry_transforms: a discrete symmetry must have 16 numbers")
        disc.append(m.reshape(4, 4))
    cont = []
    steps = int(math.ceil(math.pi / max_sym_disc_step))
    for sym in model_info.get("symmetries_continuous", ()) or ():
        offset = np.asarray(sym.get("offset", (0.0, 0.0, 0.0)), np.float64).reshape(3)
        for i in range(steps):
            R = _axis_rotation(sym["axis"], i * 2.0 * math.pi / steps) if i else np.eye(3)
            cont.append((R, offset - R @ offset))
    out = []
    for d in disc:
        if not cont:
            out.append(d)
        for Rc, tc in cont:
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = Rc @ d[:3, :3], Rc @ d[:3, 3] + tc
            out.append(m)
    out = np.ascontiguousarray(np.stack(out), np.float64)
    out[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    return out


# ------------------------------------------------------------------------------------------------ the two entry points
def pose_workspace_bytes(N, S):
    return _eval.value("gpe_pose_workspace_bytes", N, S)


@torch.no_grad()
def mssd_mspd(vertices, syms, est, gt, K, zmin=0.0, workspace=None):
    """gpe_mssd_mspd: vertices f32 (V,3), syms f64 (S,4,4), est, gt f64 (N,4,4), K f64 (N,9) on the device -> the SQUARED
    errors mssd2, mspd2 f64 (N,) on the device.  N <= 65535.  `workspace`: int64, at least pose_workspace_bytes(N, S) bytes."""
    who = "mssd_mspd"
    vertices = _lib.arg(vertices, torch.float32, (None, 3), who, "vertices")
    syms = _lib.arg(syms, torch.float64, (None, 4, 4), who, "syms")
    est = _lib.arg(est, torch.float64, (None, 4, 4), who, "est")
    N, V, S = est.shape[0], vertices.shape[0], syms.shape[0]
    gt = _lib.arg(gt, torch.float64, (N, 4, 4), who, "gt")
    K = _lib.arg(K, torch.float64, (N, 9), who, "K")
    if V < 1 or S < 1:
        raise ValueError(f"{who}: needs at least one vertex and one symmetry transform (the identity), got V = {V}, S = {S}")
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: pose_errors chunks)")
    if not math.isfinite(zmin):
        raise ValueError(f"{who}: zmin must be finite")
    need = N * S * 14 * 8
    if workspace is None:
        _lib.on_gpu(who, est=est)
        workspace = torch.empty(max(1, need // 8), dtype=torch.int64, device=est.device)
    workspace = _lib.arg(workspace, torch.int64, (None,), who, "workspace")
    if workspace.numel() * 8 < need:
        raise ValueError(f"{who}: the workspace is too small ({workspace.numel() * 8} < {need} bytes)")
    _lib.on_gpu(who, vertices=vertices, syms=syms, est=est, gt=gt, K=K, workspace=workspace)
    mssd2 = torch.empty(N, dtype=torch.float64, device=est.device)
    mspd2 = torch.empty(N, dtype=torch.float64, device=est.device)
    _call("gpe_mssd_mspd", vertices, V, syms, S, est, gt, K, N, zmin, mssd2, mspd2, workspace, _lib.stream_ptr())
    return mssd2, mspd2


def _host_index(idx, N, limit, who, what):
    """An index array on the host, checked against its range BEFORE it is uploaded."""
    if isinstance(idx, torch.Tensor):
        if idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{who}: {what} must be an integer tensor, got {idx.dtype}")
        idx = idx.detach().cpu().numpy()
    idx = np.asarray(idx)
    if idx.dtype.kind not in "iu" or idx.shape != (N,):
        raise ValueError(f"{who}: expected {what} integers ({N},), got {idx.dtype} {idx.shape}")
    if N and (int(idx.min()) < 0 or int(idx.max()) >= limit):
        raise ValueError(f"{who}: a {what} index lies outside [0, {limit})")
    return np.ascontiguousarray(idx, np.int32)


@torch.no_grad()
def vsd_counts(depth_est, depth_gt, depth_test, frame, ray, ray_index, delta, thr):
    """gpe_vsd_counts: depth_est, depth_gt f32 (N,H,W), depth_test f32 (M,H,W), ray f64 (R,H,W), thr f64 (N,T) on the device;
    frame, ray_index (N,) integers on the host or the device (checked against M, R on the host) -> counts int64 (N, 2+T) on the
    device: union, intersection, bad[t].  N <= 65535, T <= 16."""
    who = "vsd_counts"
    depth_est = _lib.arg(depth_est, torch.float32, (None, None, None), who, "depth_est")
    N, H, W = depth_est.shape
    depth_gt = _lib.arg(depth_gt, torch.float32, (N, H, W), who, "depth_gt")
    depth_test = _lib.arg(depth_test, torch.float32, (None, H, W), who, "depth_test")
    ray = _lib.arg(ray, torch.float64, (None, H, W), who, "ray")
    thr = _lib.arg(thr, torch.float64, (N, None), who, "thr")
    M, R, T = depth_test.shape[0], ray.shape[0], thr.shape[1]
    if not 1 <= T <= MAX_THRESHOLDS:
        raise ValueError(f"{who}: T = {T} thresholds (1 to {MAX_THRESHOLDS})")
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: vsd_errors chunks)")
    if H < 1 or W < 1 or H * W >= 2 ** 31 or M < 1 or R < 1:
        raise ValueError(f"{who}: bad sizes (H, W > 0, H*W < 2^31, M, R >= 1)")
    if math.isnan(delta):
        raise ValueError(f"{who}: delta is NaN")
    frame, ray_index = _host_index(frame, N, M, who, "frame"), _host_index(ray_index, N, R, who, "ray_index")
    _lib.on_gpu(who, depth_est=depth_est, depth_gt=depth_gt, depth_test=depth_test, ray=ray, thr=thr)
    dev = depth_est.device
    frame, ray_index = torch.from_numpy(frame).to(dev), torch.from_numpy(ray_index).to(dev)
    counts = torch.empty(N, 2 + T, dtype=torch.int64, device=dev)
    _call("gpe_vsd_counts", depth_est, depth_gt, N, depth_test, M, frame, ray, R, ray_index, H, W, delta, thr, T, counts, _lib.stream_ptr())
    return counts


# ------------------------------------------------------------------------------------------------ errors of any number of pairs
def _cameras(K, N, who):
    K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    K = np.asarray(K, np.float64)
    if K.shape in ((3, 3), (9,)):
        K = np.broadcast_to(K.reshape(1, 9), (N, 9))
    if K.shape not in ((N, 3, 3), (N, 9)):
        raise ValueError(f"{who}: expected K (N,3,3), (N,9) or one (3,3) with N = {N}, got {K.shape}")
    return np.ascontiguousarray(K.reshape(N, 9))


@torch.no_grad()
def pose_errors(vertices, syms, est, gt, K, zmin=0.0, device="cuda"):
    """vertices (V,3), syms (S,4,4), est, gt (N,4,4) object -> camera in the units of the vertices, K (N,3,3) or one (3,3); numpy
    or tensors anywhere -> mssd, mspd: torch float64 (N,) on the HOST (+inf for a pair with a non-finite value, mspd also with a
    vertex whose depth is below zmin on either side).  The kernels return the squares; the roots are numpy's, on the host."""
    who = "pose_errors"
    vertices = _lib.checked(vertices, torch.float32, (None, 3), who, "vertices")
    syms = _lib.checked(syms, torch.float64, (None, 4, 4), who, "syms")
    est = _lib.checked(est, torch.float64, (None, 4, 4), who, "est")
    N, S = est[0].shape[0], syms[0].shape[0]
    gt = _lib.checked(gt, torch.float64, (N, 4, 4), who, "gt")
    Kh = _cameras(K, N, who)
    if vertices[0].shape[0] < 1 or S < 1:
        raise ValueError(f"{who}: needs at least one vertex and one symmetry transform (the identity)")
    if not math.isfinite(zmin):
        raise ValueError(f"{who}: zmin must be finite")
    vertices, syms, est, gt = _lib.upload(who, device, vertices, syms, est, gt)
    Kd = torch.from_numpy(Kh).to(device)
    step = max(1, min(MAX_PAIRS_PER_CALL, WORKSPACE_BYTES_PER_CALL // (S * 14 * 8)))
    work = torch.empty(max(1, min(N, step) * S * 14), dtype=torch.int64, device=device)
    d2, p2 = torch.empty(N, dtype=torch.float64, device=device), torch.empty(N, dtype=torch.float64, device=device)
    for _, a, b in _lib.chunked(N, step):
        d2[a:b], p2[a:b] = mssd_mspd(vertices, syms, est[a:b], gt[a:b], Kd[a:b], zmin, workspace=work)
    return torch.from_numpy(np.sqrt(d2.cpu().numpy())), torch.from_numpy(np.sqrt(p2.cpu().numpy()))


def ray_map(K, H, W):
    """(H,W) float64 on the host: the length of the viewing ray through each pixel at unit depth (gigapose_eval.h)."""
    K = np.asarray(K, np.float64).reshape(9)
    a = (np.arange(W, dtype=np.float64)[None, :] - K[2]) / K[0]
    b = (np.arange(H, dtype=np.float64)[:, None] - K[5]) / K[4]
    return np.sqrt((a * a + b * b) + 1.0)


def vsd_from_counts(counts):
    """counts (N, 2+T) int64 on the host -> e (N,T) float64: (bad + union - intersection) / union, 1.0 where the union is empty."""
    c = np.asarray(counts, np.int64)
    union, inter, bad = c[:, 0:1], c[:, 1:2], c[:, 2:]
    with np.errstate(all="ignore"):
        e = (bad + union - inter).astype(np.float64) / union.astype(np.float64)
    return np.where(union == 0, 1.0, e)


@torch.no_grad()
def vsd_errors(mesh, est, gt, K, depth_test, frame, diameter, delta=15.0, taus=TAUS, H=480, W=640, znear=1e-3, device="cuda",
               views_per_call=None):
    """mesh = (vertices (V,3), faces (F,3)[, ...]); est, gt (N,4,4); K (N,3,3) or one (3,3); depth_test (M,H,W) f32, the sensor's
    z-depth in the units of the mesh (0 = no measurement); frame (N,) into M; diameter a number or (N,); delta in the same units.
    Both pose sets are drawn with MeshRenderer (pairs grouped by K, views chunked); no depth map crosses PCIe.  ->
      "errors"  (N,T) torch f64 on the host, one column per tau;   "counts" (N, 2+T) torch int64 on the host;
      "clipped" (N,) torch bool: the ESTIMATE dropped a triangle (a vertex behind znear, off beyond 16384 px or not finite) -- its
                errors are 1.0 for every tau.  A clipped GROUND TRUTH raises ValueError."""
    who = "vsd_errors"
    vertices = _lib.checked(mesh[0], torch.float32, (None, 3), who, "vertices")
    faces = _lib.checked(mesh[1], torch.int32, (None, 3), who, "faces")
    est64 = _lib.checked(est, torch.float64, (None, 4, 4), who, "est")
    N = est64[0].shape[0]
    gt64 = _lib.checked(gt, torch.float64, (N, 4, 4), who, "gt")
    Kh = _cameras(K, N, who)
    depth_test = _lib.checked(depth_test, torch.float32, (None, H, W), who, "depth_test")
    frame = _host_index(frame, N, depth_test[0].shape[0], who, "frame")
    taus = np.asarray(taus, np.float64).reshape(-1)
    T = len(taus)
    if not 1 <= T <= MAX_THRESHOLDS:
        raise ValueError(f"{who}: {T} taus (1 to {MAX_THRESHOLDS})")
    diameter = np.asarray(diameter, np.float64)
    if diameter.shape not in ((), (N,)):
        raise ValueError(f"{who}: diameter must be a number or ({N},), got {diameter.shape}")
    diameter = np.broadcast_to(diameter, (N,))
    vertices, faces, est64, gt64, depth_test = _lib.upload(who, device, vertices, faces, est64, gt64, depth_test)
    thr = torch.from_numpy(np.ascontiguousarray(taus[None, :] * diameter[:, None])).to(device)
    est32, gt32 = est64.to(torch.float32), gt64.to(torch.float32)
    counts = torch.zeros(N, 2 + T, dtype=torch.int64, device=device)
    clipped = torch.zeros(N, dtype=torch.int32, device=device)
    if views_per_call is None:
        views_per_call = max(1, DEPTH_BYTES_PER_CALL // (H * W * 4))
    step = max(1, min(int(views_per_call), MAX_PAIRS_PER_CALL))
    groups = {}
    for n in range(N):
        groups.setdefault(Kh[n].tobytes(), []).append(n)
    for idx in groups.values():
        Kg = Kh[idx[0]]
        renderer = MeshRenderer(H, W, Kg.reshape(3, 3), znear)
        ray = torch.from_numpy(ray_map(Kg, H, W)[None]).to(device)
        for _, a, b in _lib.chunked(len(idx), step):
            sel = torch.as_tensor(idx[a:b], dtype=torch.int64, device=device)
            r_est = renderer(vertices, faces, None, est32[sel], views_per_call=step, colour=(255, 255, 255), on_clipped="ignore")
            r_gt = renderer(vertices, faces, None, gt32[sel], views_per_call=step, colour=(255, 255, 255), on_clipped="ignore")
            bad_gt = torch.nonzero(r_gt["clipped"]).flatten().tolist()
            if bad_gt:
                raise ValueError(f"{who}: the ground truth of pair {idx[a + bad_gt[0]]} drops {int(r_gt['clipped'][bad_gt[0]])} triangles "
                                 f"(a vertex behind znear = {znear}, beyond 16384 px or not finite): there is no near-plane clipping")
            counts[sel] = vsd_counts(r_est["depth"], r_gt["depth"], depth_test, frame[idx[a:b]], ray, np.zeros(b - a, np.int32), delta,
                                     thr[sel].contiguous())
            clipped[sel] = r_est["clipped"]
    counts, clipped = counts.cpu().numpy(), clipped.cpu().numpy() != 0
    errors = vsd_from_counts(counts)
    errors[clipped] = 1.0
    return {"errors": torch.from_numpy(errors), "counts": torch.from_numpy(counts), "clipped": torch.from_numpy(clipped)}


# ------------------------------------------------------------------------------------------------ matching and recall (host)
def match_greedy(errors, threshold, valid=None):
    """errors (E,G): estimates in descending score x ground truths.  Each estimate in turn takes the still-unmatched ground truth
    with the smallest error (the lowest index on a tie) if that error is below the threshold; -> the number of matched ground truths.
    valid (G,) bool: every ground truth takes part in the matching (one that is not valid still absorbs its estimate), only the
    valid ones are counted."""
    errors = np.asarray(errors, np.float64)
    free = np.ones(errors.shape[1], bool)
    for e in errors:
        if not free.any():
            break
        cand = np.where(free, e, np.inf)
        g = int(np.argmin(cand))
        if free[g] and cand[g] < threshold:
            free[g] = False
    if valid is not None:
        return int((~free & np.asarray(valid, bool).reshape(-1)).sum())
    return int((~free).sum())


def read_estimates(path):
    """The csv inout.save_predictions_from_batched_predictions writes (either file) -> a list of dicts in file order."""
    import pandas as pd

    out = []
    for row in pd.read_csv(path, float_precision="round_trip").itertuples():
        R = np.asarray(str(row.R).split(), np.float64)
        t = np.asarray(str(row.t).split(), np.float64)
        if R.size != 9 or t.size != 3:
            raise ValueError(f"read_estimates: {path}: a row's R / t does not hold 9 / 3 numbers")
        out.append(dict(scene_id=int(row.scene_id), im_id=int(row.im_id), obj_id=int(row.obj_id), score=float(row.score), R=R.reshape(3, 3), t=t))
    return out


def group_estimates(targets, gts, estimates):
    """The grouping rule of the scorers (PoseScorer, distances.AddScorer): per target the inst_count highest-scored estimates of
    that object in that image (a tie in score: file order) and every ground truth of it there
    -> [(target, [estimates kept, descending score], [ground truths])]."""
    by_key = {}
    for i, e in enumerate(estimates):
        by_key.setdefault((int(e["scene_id"]), int(e["im_id"]), int(e["obj_id"])), []).append((-float(e["score"]), i, e))
    out = []
    for t in targets:
        key = (int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"]))
        kept = [e for _, _, e in sorted(by_key.get(key, []), key=lambda r: r[:2])][:int(t["inst_count"])]
        g = [g for g in gts.get(key[:2], []) if int(g["obj_id"]) == key[2]]
        out.append((t, kept, g))
    return out


def visibilities(who, ground_truths):
    """The "visib_fract" of each ground truth of one target -> float64 (G,); a ground truth without the key raises (min_visib
    needs gtinfo.with_visibility, or scene_gt_info.json's value)."""
    for g in ground_truths:
        if g.get("visib_fract") is None:
            raise ValueError(f"{who}: min_visib is set and a ground truth of object {g['obj_id']} has no 'visib_fract' "
                             "(gtinfo.with_visibility adds it)")
    return np.asarray([float(g["visib_fract"]) for g in ground_truths], np.float64).reshape(-1)


def check_min_visib(who, min_visib):
    if min_visib is not None and not 0 <= float(min_visib) <= 1:
        raise ValueError(f"{who}: min_visib must be None or lie in [0, 1], got {min_visib!r}")
    return None if min_visib is None else float(min_visib)


class PoseScorer:
    """BOP-19 recall of a set of estimates.
      models   {obj_id: {"vertices" (V,3), "faces" (F,3), "diameter", ["symmetries_discrete"], ["symmetries_continuous"]}}
      targets  [{"scene_id", "im_id", "obj_id", "inst_count"}]             (test_targets_bop19.json)
      gts      {(scene_id, im_id): [{"obj_id", "cam_R_m2c" 9, "cam_t_m2c" 3, ["visib_fract"]}]}   (scene_gt.json [+ scene_gt_info.json])
      cameras  {(scene_id, im_id): {"cam_K" 9, "depth" (H,W) z-depth in the units of the models, 0 = no measurement}}
      min_visib  None: every listed instance counts.  A number (BOP-19: 0.1): a ground truth whose "visib_fract" is below it
               still takes part in the greedy matching -- it absorbs the estimate that lands on it -- but is counted neither
               among the matched nor in "targets"; a ground truth without the key raises (gtinfo.GroundTruthInfo computes it,
               gtinfo.with_visibility adds it)
    Per target it keeps the inst_count highest-scored estimates, computes the three errors of every estimate x ground truth of that
    object in that image on the GPU, and matches greedily per threshold on the host (match_greedy).  Recall = matched ground
    truths / ground truths of all targets."""

    def __init__(self, models, targets, gts, cameras, delta=15.0, taus=TAUS, max_sym_disc_step=0.01, znear=1e-3, device="cuda", min_visib=None):
        self.models, self.targets, self.gts = models, list(targets), gts
        self.min_visib = check_min_visib("PoseScorer", min_visib)
        self.delta, self.taus, self.znear, self.device = float(delta), tuple(taus), float(znear), device
        self.syms = {o: symmetry_transforms(m, max_sym_disc_step) for o, m in models.items()}
        self._table = CameraTable("PoseScorer", cameras, "required", max_pixels=None)
        self.frames, self.H, self.W, self.K = self._table.frames, self._table.H, self._table.W, self._table.K
        for t in self.targets:
            key = (int(t["scene_id"]), int(t["im_id"]))
            if key not in self._table.index:
                raise ValueError(f"PoseScorer: target image {key} has no camera")
            if int(t["obj_id"]) not in models:
                raise ValueError(f"PoseScorer: target object {t['obj_id']} has no model")

    def score_csv(self, path):
        return self.score(read_estimates(path))

    def pairs(self, estimates):
        """-> per target [(target, [estimates kept, descending score], [ground truths])]."""
        return group_estimates(self.targets, self.gts, estimates)

    def errors(self, estimates):
        """-> [(target, {"mssd" (E,G), "mspd" (E,G), "vsd" (E,G,T), "clipped" (E,G)})] as numpy, E estimates kept x G ground truths;
        with min_visib also "visib" (G,), the ground truths' visib_fract."""
        groups = self.pairs(estimates)
        visib = None if self.min_visib is None else [visibilities("PoseScorer", g) for _, _, g in groups]     # raises before any GPU work
        depth = self._table.depth_on(self.device)
        out = [None] * len(groups)
        for obj in sorted({int(t["obj_id"]) for t, _, _ in groups}):
            est, gt, K, frame, where = [], [], [], [], []
            for gi, (t, kept, g) in enumerate(groups):
                if int(t["obj_id"]) != obj:
                    continue
                key = (int(t["scene_id"]), int(t["im_id"]))
                where.append((gi, len(est), len(kept), len(g)))
                for e in kept:
                    for h in g:
                        est.append(pose_matrix(e["R"], e["t"]))
                        gt.append(pose_matrix(h["cam_R_m2c"], h["cam_t_m2c"]))
                        K.append(self.K[key])
                        frame.append(self._table.index[key])
            T = len(self.taus)
            if est:
                m = self.models[obj]
                est, gt, K = np.stack(est), np.stack(gt), np.stack(K)
                mssd, mspd = (a.numpy() for a in pose_errors(m["vertices"], self.syms[obj], est, gt, K, self.znear, self.device))
                vsd = vsd_errors((m["vertices"], m["faces"]), est, gt, K, depth, np.asarray(frame), float(m["diameter"]), self.delta,
                                 self.taus, self.H, self.W, self.znear, self.device)
                e_vsd, clipped = vsd["errors"].numpy(), vsd["clipped"].numpy()
            for gi, o, E, G in where:
                sl = slice(o, o + E * G)
                if E * G:
                    out[gi] = (groups[gi][0], dict(mssd=mssd[sl].reshape(E, G), mspd=mspd[sl].reshape(E, G), vsd=e_vsd[sl].reshape(E, G, T),
                                                   clipped=clipped[sl].reshape(E, G)))
                else:
                    out[gi] = (groups[gi][0], dict(mssd=np.zeros((E, G)), mspd=np.zeros((E, G)), vsd=np.zeros((E, G, T)),
                                                   clipped=np.zeros((E, G), bool)))
        if visib is not None:
            for (_, e), v in zip(out, visib):
                e["visib"] = v
        return out

    def score(self, estimates):
        return recall_from_errors(self.errors(estimates), {o: float(m["diameter"]) for o, m in self.models.items()}, self.W, self.min_visib)


def counted(per_target, min_visib, table="mssd"):
    """Per target the ground truths that count: None (all of them: the columns of errors[table]) without min_visib, else
    errors["visib"] >= min_visib; and their number."""
    if min_visib is None:
        return [None] * len(per_target), sum(e[table].shape[1] for _, e in per_target)
    valid = [np.asarray(e["visib"], np.float64) >= float(min_visib) for _, e in per_target]
    return valid, int(sum(int(v.sum()) for v in valid))


def recall_from_errors(per_target, diameters, W, min_visib=None):
    """[(target, errors)] as PoseScorer.errors returns them -> {"recall_mssd" [10], "recall_mspd" [10], "recall_vsd" [T][10],
    "ar_mssd", "ar_mspd", "ar_vsd", "ar", "targets": ground truths counted, "clipped": estimates x ground truths reported clipped}.
    min_visib: only the ground truths with errors["visib"] >= min_visib are counted, in the matches and in "targets"."""
    r = W / 640.0
    valid, total = counted(per_target, min_visib)
    T = per_target[0][1]["vsd"].shape[2] if per_target else 0
    tp_mssd, tp_mspd = np.zeros(len(CORRECT_THS), np.int64), np.zeros(len(MSPD_THS), np.int64)
    tp_vsd = np.zeros((T, len(CORRECT_THS)), np.int64)
    for (t, e), ok in zip(per_target, valid):
        d = diameters[int(t["obj_id"])]
        for i, th in enumerate(CORRECT_THS):
            tp_mssd[i] += match_greedy(e["mssd"], th * d, ok)
            for k in range(T):
                tp_vsd[k, i] += match_greedy(e["vsd"][:, :, k], th, ok)
        for i, th in enumerate(MSPD_THS):
            tp_mspd[i] += match_greedy(e["mspd"], th * r, ok)
    den = float(max(total, 1))
    out = dict(recall_mssd=(tp_mssd / den).tolist(), recall_mspd=(tp_mspd / den).tolist(), recall_vsd=(tp_vsd / den).tolist(), targets=total,
               clipped=int(sum(int(e["clipped"].sum()) for _, e in per_target)))
    out["ar_mssd"], out["ar_mspd"] = float(np.mean(out["recall_mssd"])), float(np.mean(out["recall_mspd"]))
    out["ar_vsd"] = float(np.mean(out["recall_vsd"])) if T else 0.0
    out["ar"] = (out["ar_mssd"] + out["ar_mspd"] + out["ar_vsd"]) / 3.0
    return out
