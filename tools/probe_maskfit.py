"""Silhouette fit measurement (needs one MI355X): gpm_moments beside gpv_counts with masks on the same keys and boxes, at the
shape of profiles/verify_hypotheses.txt; gpm_mask_moments, gpm_update and a whole MaskRefiner.refine beside them.

Workload (seeded, generated here; tools/probe_verify.py's): --pairs 1 500 estimates of one object (an icosphere(5)-sized mesh,
20 480 faces) on one 480 x 640 frame; the estimates are the true pose moved by up to 4 degrees and 4 % of the diameter; boxes are
the projected model's bounding boxes padded by 8 pixels; one mask per 5 pairs (the silhouette of the true pose as run lengths,
one list per detection); the pairs chunked as MaskRefiner chunks them (the keys of a call below 1 GiB).  Per repetition every
chunk is drawn once and three kernels run on its keys with HIP events around each, summed over the chunks: gpm_moments,
gpv_counts with masks and no depth (the RGB-only score), gpv_counts with masks and depth; their order alternates from repetition
to repetition.  gpm_mask_moments (all masks, one call) and gpm_update (all pairs of a chunk, summed) are timed in the same
repetitions.  --reps repetitions after --warmup warm-ups.

No time is required of any of these: there is no earlier code to compare with, and this file records what was measured.  The
run fails only if the rows of the first --host-pairs pairs or the masks' moments differ from the restatement.  The wall time of
MaskRefiner.refine over all pairs (8 steps; render and host work included) is recorded.  Writes --out (default
profiles/maskfit_silhouette.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import _lib, ingest, maskfit, refine, render, verify  # noqa: E402
from gigapose_testing import maskfit_ref, meshes  # noqa: E402
from gigapose_testing import refine_cases as cases  # noqa: E402

DEV = "cuda"
H, W = 480, 640
K = np.asarray([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stats(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[0]), float(v[-1])


class Stage:
    """HIP events around every call of one stage; .ms() after a synchronisation."""

    def __init__(self):
        self.events = []

    def __call__(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.events.append((a, b))
        return out

    def ms(self):
        total = sum(a.elapsed_time(b) for a, b in self.events)
        self.events = []
        return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskfit_silhouette.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--level", type=int, default=5, help="subdivisions of the icosphere")
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--refine-reps", type=int, default=3)
    args = ap.parse_args()
    rs = np.random.RandomState(7)
    v, f, _ = meshes.icosphere(args.level, 1.0)
    v = (v.astype(np.float64) * (60.0, 45.0, 30.0) * (1.0 + 0.15 * np.sin(4.0 * v[:, [1, 2, 0]]))).astype(np.float32)
    diameter = float(2 * np.linalg.norm(v, axis=1).max())
    gt = cases.rigid(cases.rot([1, 2, 3], 35), (30.0, -20.0, 600.0))
    N = args.pairs
    starts = np.stack([cases.moved(gt, rs.standard_normal(3), rs.uniform(0, 4), rs.uniform(-0.04, 0.04, 3) * diameter) for _ in range(N)])
    Kn = np.tile(K, (N, 1))
    box = refine.projected_boxes(v, starts, Kn, H, W, 8.0)
    clamped = np.stack([np.maximum(box[:, 0], 0), np.maximum(box[:, 1], 0), np.minimum(box[:, 2], W - 1), np.minimum(box[:, 3], H - 1)], axis=1)
    box_pixels = int((np.maximum(clamped[:, 2] - clamped[:, 0] + 1, 0).astype(np.int64) * np.maximum(clamped[:, 3] - clamped[:, 1] + 1, 0)).sum())

    vd, fd = dev(v), dev(f)
    truth = render.MeshRenderer(H, W, K)(vd, fd, None, dev(gt[None].astype(np.float32)), colour=(255, 255, 255))["depth"]
    depth = torch.round(torch.where(truth > 0, truth, torch.full_like(truth, 900.0)))
    runs = ingest.mask_to_rle_counts((truth[0] > 0).cpu().numpy())
    D = -(-N // 5)
    counts_h, offsets_h = np.tile(runs, D), (np.arange(D + 1) * len(runs)).astype(np.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    offsets_d = dev(offsets_h)
    masks = (ingest.RleDetectionPreprocessor().scan(dev(counts_h), offsets_d, H, W, err), offsets_d)
    assert err.item() == 0
    det_h = (np.arange(N) // 5).astype(np.int32)
    det = dev(det_h)
    step = max(1, min(render.VIS_BYTES_PER_CALL // (H * W * 8), maskfit.MAX_PAIRS_PER_CALL))
    chunks = [(a, b) for _, a, b in _lib.chunked(N, step)]
    V, F = v.shape[0], f.shape[0]
    K9 = render._k9(K)
    buffers = render.KeyBuffers(min(N, step), V, F, H, W, DEV)
    start, Kd, boxd = dev(starts), dev(Kn), dev(box)
    poses32 = start.to(torch.float32)
    frame = torch.zeros(N, dtype=torch.int32, device=DEV)
    tol = torch.full((N,), 0.05 * diameter, dtype=torch.float64, device=DEV)
    mrows = torch.empty(N, maskfit.ROW, dtype=torch.int64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    crows = {k: (torch.empty(N, verify.COUNTS, dtype=torch.int64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)) for k in ("masked", "masked_depth")}
    clipped = torch.empty(N, dtype=torch.int32, device=DEV)
    moved, moved32 = torch.empty_like(start), torch.empty_like(poses32)
    best, score, state = maskfit.new_state(N, DEV)
    stages = {k: Stage() for k in ("render", "moments", "masked", "masked_depth", "mask_moments", "update")}
    kept = {}

    def run(rep):
        kept["mm"] = stages["mask_moments"](lambda: maskfit.mask_moments(masks, H, W))
        moved.copy_(start), moved32.copy_(poses32)
        for a, b in chunks:
            keys = stages["render"](lambda: buffers.draw(vd, fd, poses32[a:b], K9, 1e-3, clipped[a:b])[0])
            work_ = {"moments": lambda: maskfit.moments(keys, masks, det[a:b], boxd[a:b], out=(mrows[0][a:b], mrows[1][a:b])),
                     "masked": lambda: verify.counts(keys, None, None, masks, det[a:b], boxd[a:b], tol[a:b], out=(crows["masked"][0][a:b], crows["masked"][1][a:b])),
                     "masked_depth": lambda: verify.counts(keys, depth, frame[a:b], masks, det[a:b], boxd[a:b], tol[a:b],
                                                           out=(crows["masked_depth"][0][a:b], crows["masked_depth"][1][a:b]))}
            order = ("moments", "masked", "masked_depth")
            for name in order[rep % 3:] + order[:rep % 3]:
                stages[name](work_[name])
            stages["update"](lambda: maskfit.update(mrows[0][a:b], mrows[1][a:b], kept["mm"][0], det[a:b], clipped[a:b], Kd[a:b], start[a:b], 0, False, moved[a:b],
                                                    moved32[a:b], best[a:b], score[a:b], state[a:b]))
            if rep == 0 and a == 0:
                kept["vis"] = keys[:args.host_pairs].cpu().numpy()
        torch.cuda.synchronize()

    times = {k: [] for k in stages}
    for rep in range(args.warmup + args.reps):
        run(rep)
        for k in stages:
            t = stages[k].ms()
            if rep >= args.warmup:
                times[k].append(t)

    hp = args.host_pairs
    cum = np.tile(np.cumsum(runs), D).astype(np.int32)
    want = maskfit_ref.moments(kept["vis"].view(np.uint64), cum, offsets_h, det_h[:hp], box[:hp])
    want_mm = maskfit_ref.mask_moments(cum[:len(runs)], offsets_h[:2], H, W)
    mm = kept["mm"][0].cpu().numpy()
    same = (want[0].tobytes() == mrows[0][:hp].cpu().numpy().tobytes() and not mrows[1].any().item() and not kept["mm"][1].any().item()
            and (mm == want_mm[0][0]).all())
    inter = mrows[0][:, maskfit.INTER].sum().item() / max(1, crows["masked"][0][:, 1].sum().item())
    moved_pairs = int(((state[:, 0] & maskfit.STOP) == 0).sum().item())

    models = {1: dict(vertices=v, faces=f, diameter=diameter)}
    cameras = {(1, 1): dict(cam_K=K, size=(H, W))}
    est = [dict(scene_id=1, im_id=1, obj_id=1, score=float(rs.uniform()), R=p[:3, :3].copy(), t=p[:3, 3].copy(), instance_id=i // 5) for i, p in enumerate(starts)]
    seg = dict(size=[H, W], counts=runs.tolist())
    segs = {d: seg for d in range(D)}
    fitter = maskfit.MaskRefiner(models, cameras)
    wall = []
    for rep in range(1 + args.refine_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fitted = fitter.refine(est, segs)
        wall.append((time.perf_counter() - t0) * 1e3)
    iou0, iou1 = np.asarray([e["iou_start"] for e in fitted]), np.asarray([e["iou"] for e in fitted])
    improved = int(sum(e["best_iteration"] > 0 for e in fitted))

    mom, msk = stats(times["moments"]), stats(times["masked"])
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each call (its memsets included), summed over the {len(chunks)} chunks of a "
             "repetition; times in ms: median (min .. max)",
             f"workload: {N} estimates of one object ({V} vertices, {F} faces, diameter {diameter:.1f}) on a {H} x {W} frame, {step} pairs per call; boxes hold "
             f"{box_pixels / N:.0f} pixels on average ({100.0 * box_pixels / (N * H * W):.1f}% of the frame); {D} masks of {len(runs)} runs, one per 5 pairs", ""]
    for name, label in (("render", "render"), ("moments", "gpm_moments"), ("masked", "gpv_counts + masks"), ("masked_depth", "gpv_counts + masks + depth"),
                        ("mask_moments", f"gpm_mask_moments ({D})"), ("update", f"gpm_update ({N})")):
        m, lo, hi = stats(times[name])
        lines.append(f"   {label:<26}: {m:9.3f} ms ({lo:.3f} .. {hi:.3f})")
    lines += ["", f"gpm_moments: {box_pixels:.3e} box pixels, {8.0 * box_pixels / 1e9:.2f} GB of keys -> {8.0 * box_pixels / (mom[0] * 1e-3) / 1e9:.1f} GB/s (a bisection of "
              f"{len(runs)} prefix sums per COVERED pixel); gpv_counts with masks and no depth on the same keys and boxes: {8.0 * box_pixels / (msk[0] * 1e-3) / 1e9:.1f} GB/s "
              f"(a bisection per box pixel); gpm_moments takes {mom[0] / msk[0]:.2f}x its time.  No time is required: recorded, not bounded.",
              f"   the first {hp} pairs' rows and the masks' moments equal the restatement bit for bit and no status bit is set: {same}",
              f"   the intersections of gpm_moments sum to {inter:.6f}x the covered-in-mask counts of gpv_counts (1 = the same pixels); {moved_pairs} of {N} pairs took a step",
              f"MaskRefiner.refine over {N} estimates of {D} detections, 8 steps (host work, uploads, 9 x (project, raster, moments, update), read-back; wall clock, "
              f"{args.refine_reps} runs after one): median {np.median(wall[1:]):.1f} ms (min {min(wall[1:]):.1f}) = {1e3 * N / np.median(wall[1:]):.0f} estimates per second",
              f"   IoU with the mask: mean {iou0.mean():.4f} -> {iou1.mean():.4f}, least {iou0.min():.4f} -> {iou1.min():.4f}; {improved} of {N} estimates improved"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not same:
        raise SystemExit("the device rows differ from the restatement")


if __name__ == "__main__":
    main()
