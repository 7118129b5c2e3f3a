"""ADD, ADD-S and the model diameter ON the GPU (libgigapose_dist.so, C-ABI: include/gigapose_dist.h, which spells the arithmetic
out; gigapose_testing/dist_ref.py restates it in numpy and tests/test_gpu_dist.py holds the kernels to it bit for bit).

ADD is the mean distance between a model's vertices under the estimate and the same vertices under the ground truth, ADD-S the
mean distance from each ground-truth vertex to the NEAREST estimate vertex (Hinterstoisser et al., ACCV 2012): the numbers LM,
LM-O and YCB-V tables are written in, as recall at 0.1 x diameter and as the area under the accuracy curve.  The diameter -- the
largest distance between two vertices -- is what every threshold of the scorers is a multiple of; a mesh that comes through
render.load_ply has none.  ADD-S and the diameter visit all pairs of vertices: O(V^2) per item, a float64 vector-ALU hot path.
The means are taken over INTEGERS (distances quantised to 2^-k units), so their bits depend on no summation order.

  add_sums(vertices, est, gt, symmetric, k=20)         the entry points on device tensors, <= 65535 pairs -> sums, status
  add_errors(vertices, est, gt, symmetric=False, ...)  any number of pairs, anything anywhere -> {"errors", "status"} on the host
  model_diameter(vertices)                             -> float
  AddScorer(models, targets, gts)                      .score_csv(path) / .score(estimates) -> recalls at 0.1 d and AUCs
Out of scope: a KD-tree for very large models (the all-pairs kernel is exact and takes V <= 2^20), ADD minimised over symmetry
transforms (MSSD of evaluate.py is the symmetry-aware error), the AUC variants of other toolkits (the definition is AddScorer's
docstring).  There is no CPU fallback: a missing library is an error.
"""
import numpy as np
import torch

from . import _lib
from .evaluate import check_min_visib, counted, group_estimates, match_greedy, pose_matrix, read_estimates, visibilities

MAX_PAIRS_PER_CALL = 65535                           # the grid's second dimension (gigapose_dist.h: Limits)
MAX_VERTICES = 1 << 20
K_RANGE = (-64, 64)
BAD_KEY = 2 ** 64 - 1
AUC_STEPS = 100
_dist = _lib.SideLibrary("libgigapose_dist.so", "gpd")
DIST_LIB_PATH, lib, _call = _dist.path, _dist.lib, _dist.call


def _check_k(who, k):
    if int(k) != k or not K_RANGE[0] <= k <= K_RANGE[1]:
        raise ValueError(f"{who}: k must be an integer in [{K_RANGE[0]}, {K_RANGE[1]}], got {k!r}")
    return int(k)


def _check_v(who, V):
    if not 1 <= V <= MAX_VERTICES:
        raise ValueError(f"{who}: V = {V} vertices (1 to 2^20)")


@torch.no_grad()
def add_sums(vertices, est, gt, symmetric, k=20):
    """gpd_add / gpd_adds (symmetric): vertices f32 (V,3), est, gt f64 (N,4,4) on the device -> sums int64 (N,), status int32 (N,)
    on the device.  N <= 65535, V <= 2^20.  The error of pair n is sums[n] / (V * 2^k) where status[n] == 0."""
    who = "add_sums"
    vertices = _lib.arg(vertices, torch.float32, (None, 3), who, "vertices")
    est = _lib.arg(est, torch.float64, (None, 4, 4), who, "est")
    N, V = est.shape[0], vertices.shape[0]
    gt = _lib.arg(gt, torch.float64, (N, 4, 4), who, "gt")
    _check_v(who, V)
    k = _check_k(who, k)
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} pairs in one call (at most {MAX_PAIRS_PER_CALL}: add_errors chunks)")
    _lib.on_gpu(who, vertices=vertices, est=est, gt=gt)
    sums = torch.empty(N, dtype=torch.int64, device=est.device)
    status = torch.empty(N, dtype=torch.int32, device=est.device)
    _call("gpd_adds" if symmetric else "gpd_add", vertices, V, est, gt, N, k, sums, status, _lib.stream_ptr())
    return sums, status


def errors_from_sums(sums, status, V, k):
    """sums, status (N,) on the host -> float64 (N,): sums / (V * 2^k), the division of Python integers (correctly rounded); +inf
    where a status bit is set."""
    num, den = (1, V << k) if k >= 0 else (1 << -k, V)
    return np.asarray([s * num / den if b == 0 else np.inf for s, b in zip(np.asarray(sums).tolist(), np.asarray(status).tolist())],
                      np.float64).reshape(-1)


@torch.no_grad()
def add_errors(vertices, est, gt, symmetric=False, k=20, device="cuda"):
    """vertices (V,3), est, gt (N,4,4) object -> camera in the units of the vertices; numpy or tensors anywhere, any N (chunked at
    65535 pairs) -> {"errors": torch float64 (N,) on the HOST, ADD (ADD-S if symmetric), +inf where status != 0;
    "status": torch int32 (N,) on the host -- bit 0: a value of the pair is not finite, bit 1: a distance left the range}.
    A distance is rounded to a multiple of 2^-k units before the mean is taken: the default k = 20 and millimetres give about
    1e-6 mm of resolution and a range of 2^22 mm (4 km); metres want the same k, a unit of micrometres a smaller one."""
    who = "add_errors"
    vertices = _lib.checked(vertices, torch.float32, (None, 3), who, "vertices")
    est = _lib.checked(est, torch.float64, (None, 4, 4), who, "est")
    N, V = est[0].shape[0], vertices[0].shape[0]
    gt = _lib.checked(gt, torch.float64, (N, 4, 4), who, "gt")
    _check_v(who, V)
    k = _check_k(who, k)
    vertices, est, gt = _lib.upload(who, device, vertices, est, gt)
    sums = torch.empty(N, dtype=torch.int64, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)
    for _, a, b in _lib.chunked(N, MAX_PAIRS_PER_CALL):
        sums[a:b], status[a:b] = add_sums(vertices, est[a:b], gt[a:b], symmetric, k)
    status = status.cpu()
    return {"errors": torch.from_numpy(errors_from_sums(sums.cpu().numpy(), status.numpy(), V, k)), "status": status}


@torch.no_grad()
def diameter2_key(vertices):
    """gpd_diameter2: vertices f32 (V,3) on the device -> int64 (1,) on the device holding the 64 bits of the key."""
    who = "diameter2_key"
    vertices = _lib.arg(vertices, torch.float32, (None, 3), who, "vertices")
    _check_v(who, vertices.shape[0])
    _lib.on_gpu(who, vertices=vertices)
    key = torch.empty(1, dtype=torch.int64, device=vertices.device)
    _call("gpd_diameter2", vertices, vertices.shape[0], key, _lib.stream_ptr())
    return key


def model_diameter(vertices, device="cuda"):
    """The largest distance between two vertices (bop_toolkit's definition of models_info.json's "diameter"), over ALL pairs, as a
    float: the square comes from the kernel, its root is numpy's.  vertices (V,3) numpy or a tensor anywhere, 1 <= V <= 2^20; one
    vertex gives 0.0; a vertex that is not finite raises ValueError."""
    who = "model_diameter"
    vertices = _lib.checked(vertices, torch.float32, (None, 3), who, "vertices")
    _check_v(who, vertices[0].shape[0])
    vertices, = _lib.upload(who, device, vertices)
    key = int(diameter2_key(vertices).cpu().numpy().view(np.uint64)[0])
    if key == BAD_KEY or not bool(torch.isfinite(vertices).all()):
        raise ValueError(f"{who}: a vertex is not finite")
    return float(np.sqrt(np.asarray([key], np.uint64).view(np.float64))[0])


@torch.no_grad()
def roots(x):
    """gpd_root: x f64 (n,) on the device -> the library's square root of every element (the correctly rounded one)."""
    x = _lib.arg(x, torch.float64, (None,), "roots", "x")
    _lib.on_gpu("roots", x=x)
    out = torch.empty_like(x)
    _call("gpd_root", x, x.shape[0], out, _lib.stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ recall and AUC (host)
def is_symmetric(model_info):
    return bool(model_info.get("symmetries_discrete")) or bool(model_info.get("symmetries_continuous"))


def recall_from_add_errors(per_target, diameters, symmetric, tau_max=100.0, min_visib=None):
    """[(target, {"add" (E,G), "adds" (E,G)})] -> the dict AddScorer.score returns.  `symmetric`: {obj_id: bool}.  min_visib: only
    the ground truths with errors["visib"] >= min_visib are counted (evaluate.recall_from_errors)."""
    valid, total = counted(per_target, min_visib, "add")
    den = float(max(total, 1))
    taus = [tau_max * j / AUC_STEPS for j in range(1, AUC_STEPS + 1)]

    def pick(t, e, which):
        if which == "add_s":
            which = "adds" if symmetric[int(t["obj_id"])] else "add"
        return e[which]

    out = {"targets": total}
    for which in ("add", "adds", "add_s"):
        out["recall_" + which] = sum(match_greedy(pick(t, e, which), 0.1 * diameters[int(t["obj_id"])], ok)
                                     for (t, e), ok in zip(per_target, valid)) / den
        curve = [sum(match_greedy(pick(t, e, which), tau, ok) for (t, e), ok in zip(per_target, valid)) / den for tau in taus]
        out["auc_" + which] = float(np.mean(curve))
    return out


class AddScorer:
    """ADD / ADD-S recall and AUC of a set of estimates.
      models   {obj_id: {"vertices" (V,3), ["diameter"], ["symmetries_discrete"], ["symmetries_continuous"]}}
      targets  [{"scene_id", "im_id", "obj_id", "inst_count"}]             (test_targets_bop19.json)
      gts      {(scene_id, im_id): [{"obj_id", "cam_R_m2c" 9, "cam_t_m2c" 3, ["visib_fract"]}]}   (scene_gt.json [+ scene_gt_info.json])
      min_visib  None: every listed instance counts; a number: as PoseScorer's -- a ground truth whose "visib_fract" is below it
               still absorbs an estimate but counts neither for nor against, one without the key raises
    No cameras are needed.  A model without "diameter" gets model_diameter(vertices).  Estimates are kept and matched as PoseScorer
    does (evaluate.group_estimates: the inst_count highest-scored estimates per target; evaluate.match_greedy per threshold).
    score() ->
      "recall_add", "recall_adds"   matched ground truths / ground truths of all targets, an estimate being correct when its
                                    error is BELOW 0.1 x diameter of its object
      "recall_add_s"                the same with ADD-S for objects that list any symmetries_discrete / symmetries_continuous
                                    entry and ADD for the others (the "ADD(-S)" of the LM / YCB-V tables)
      "auc_add", "auc_adds", "auc_add_s"   THE DEFINITION: the mean over j = 1 .. 100 of the recall at the absolute threshold
                                    tau_max * j / 100 (tau_max in the units of the models: 100 mm, the 10 cm of the YCB-V
                                    tables); no toolkit is consulted, other toolkits integrate differently
      "targets"                     ground truths counted."""

    def __init__(self, models, targets, gts, k=20, tau_max=100.0, device="cuda", min_visib=None):
        self.models, self.targets, self.gts = models, list(targets), gts
        self.min_visib = check_min_visib("AddScorer", min_visib)
        self.k, self.tau_max, self.device = _check_k("AddScorer", k), float(tau_max), device
        if not self.tau_max > 0:
            raise ValueError("AddScorer: tau_max must be positive")
        for t in self.targets:
            if int(t["obj_id"]) not in models:
                raise ValueError(f"AddScorer: target object {t['obj_id']} has no model")
        self.symmetric = {int(o): is_symmetric(m) for o, m in models.items()}
        self._diameters = {int(o): float(m["diameter"]) for o, m in models.items() if m.get("diameter") is not None}

    def diameters(self):
        for o, m in self.models.items():
            if int(o) not in self._diameters:
                self._diameters[int(o)] = model_diameter(m["vertices"], self.device)
        return self._diameters

    def score_csv(self, path):
        return self.score(read_estimates(path))

    def pairs(self, estimates):
        return group_estimates(self.targets, self.gts, estimates)

    def errors(self, estimates):
        """-> [(target, {"add" (E,G), "adds" (E,G)})] as numpy, E estimates kept x G ground truths."""
        groups = self.pairs(estimates)
        visib = None if self.min_visib is None else [visibilities("AddScorer", g) for _, _, g in groups]      # raises before any GPU work
        out = [None] * len(groups)
        for obj in sorted({int(t["obj_id"]) for t, _, _ in groups}):
            est, gt, where = [], [], []
            for gi, (t, kept, g) in enumerate(groups):
                if int(t["obj_id"]) != obj:
                    continue
                where.append((gi, len(est), len(kept), len(g)))
                for e in kept:
                    for h in g:
                        est.append(pose_matrix(e["R"], e["t"]))
                        gt.append(pose_matrix(h["cam_R_m2c"], h["cam_t_m2c"]))
            if est:
                est, gt = np.stack(est), np.stack(gt)
                v = self.models[obj]["vertices"]
                add = add_errors(v, est, gt, False, self.k, self.device)["errors"].numpy()
                adds = add_errors(v, est, gt, True, self.k, self.device)["errors"].numpy()
            for gi, o, E, G in where:
                sl = slice(o, o + E * G)
                if E * G:
                    out[gi] = (groups[gi][0], dict(add=add[sl].reshape(E, G), adds=adds[sl].reshape(E, G)))
                else:
                    out[gi] = (groups[gi][0], dict(add=np.zeros((E, G)), adds=np.zeros((E, G))))
        if visib is not None:
            for (_, e), v in zip(out, visib):
                e["visib"] = v
        return out

    def score(self, estimates):
        return recall_from_add_errors(self.errors(estimates), self.diameters(), self.symmetric, self.tau_max, self.min_visib)
