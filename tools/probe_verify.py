"""Hypothesis verification measurement (needs one MI355X): gpv_counts beside gpf_accumulate on the same keys and boxes, at the
shape of profiles/refine_depth.txt.

Workload (seeded, generated here; tools/probe_refine.py's): --pairs 1 500 estimates of one object (an icosphere(5)-sized mesh,
20 480 faces) on one 480 x 640 frame whose depth is the object at its true pose in front of a wall; the estimates are the true
pose moved by up to 4 degrees and 4 % of the diameter; boxes are the projected model's bounding boxes padded by 8 pixels; the
pairs chunked as DepthRefiner chunks them (the keys of a call below 1 GiB).  Per repetition every chunk is drawn once and three
kernels run on its keys with HIP events around each, summed over the chunks: gpf_accumulate, gpv_counts without masks, gpv_counts
with one mask per 5 pairs (the silhouette of the true pose as run lengths, one list per detection).  The order of the three
alternates from repetition to repetition.  --reps repetitions after --warmup warm-ups.

CONDITION: without masks gpv_counts reads the same keys and depth as gpf_accumulate and does a fraction of its arithmetic per
covered pixel, so its median must not exceed gpf_accumulate's median by more than the spread (max - min) of gpf_accumulate's own
repetitions in this run.  The profile says whether it held; the run fails if it did not, or if the counts of the first
--host-pairs pairs differ from the numpy restatement.  The masked time and the wall time of HypothesisVerifier.select over all
pairs (render and host work included) are recorded, not bounded.  Writes --out (default profiles/verify_hypotheses.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import _lib, ingest, refine, render, verify  # noqa: E402
from gigapose_testing import meshes, verify_ref  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_hypotheses.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--level", type=int, default=5, help="subdivisions of the icosphere")
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--select-reps", type=int, default=3)
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
    c = refine.face_normals(vd, fd)
    truth = render.MeshRenderer(H, W, K)(vd, fd, None, dev(gt[None].astype(np.float32)), colour=(255, 255, 255))["depth"]
    depth = torch.round(torch.where(truth > 0, truth, torch.full_like(truth, 900.0)))
    runs = ingest.mask_to_rle_counts((truth[0] > 0).cpu().numpy())
    D = -(-N // 5)
    counts_h, offsets_h = np.tile(runs, D), (np.arange(D + 1) * len(runs)).astype(np.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    offsets_d = dev(offsets_h)
    masks = (ingest.RleDetectionPreprocessor().scan(dev(counts_h), offsets_d, H, W, err), offsets_d)
    assert err.item() == 0
    det = dev((np.arange(N) // 5).astype(np.int32))
    step = max(1, min(render.VIS_BYTES_PER_CALL // (H * W * 8), refine.MAX_PAIRS_PER_CALL))
    chunks = [(a, b) for _, a, b in _lib.chunked(N, step)]
    V, F = v.shape[0], f.shape[0]
    K9 = render._k9(K)
    buffers = render.KeyBuffers(min(N, step), V, F, H, W, DEV)
    poses, Kd, boxd = dev(starts), dev(Kn), dev(box)
    poses32 = poses.to(torch.float32)
    frame = torch.zeros(N, dtype=torch.int32, device=DEV)
    tol = 0.05 * diameter
    gate, scale = torch.full((N,), tol, dtype=torch.float64, device=DEV), torch.full((N,), diameter, dtype=torch.float64, device=DEV)
    sums, status = torch.empty(N, refine.SUMS, dtype=torch.int64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    rows = {k: (torch.empty(N, verify.COUNTS, dtype=torch.int64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)) for k in ("counts", "masked")}
    clipped = torch.empty(N, dtype=torch.int32, device=DEV)
    stages = {k: Stage() for k in ("render", "accumulate", "counts", "masked")}
    kept = {}

    def run(rep):
        for a, b in chunks:
            keys = stages["render"](lambda: buffers.draw(vd, fd, poses32[a:b], K9, 1e-3, clipped[a:b])[0])
            work_ = {"accumulate": lambda: refine.accumulate(keys, c, poses[a:b], Kd[a:b], depth, frame[a:b], boxd[a:b], gate[a:b], scale[a:b],
                                                             out=(sums[a:b], status[a:b])),
                     "counts": lambda: verify.counts(keys, depth, frame[a:b], None, None, boxd[a:b], gate[a:b], out=(rows["counts"][0][a:b], rows["counts"][1][a:b])),
                     "masked": lambda: verify.counts(keys, depth, frame[a:b], masks, det[a:b], boxd[a:b], gate[a:b], out=(rows["masked"][0][a:b], rows["masked"][1][a:b]))}
            order = ("accumulate", "counts", "masked")
            for name in order[rep % 3:] + order[:rep % 3]:
                stages[name](work_[name])
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
    cum = np.tile(np.cumsum(runs), D)
    want = verify_ref.counts(kept["vis"].view(np.uint64), depth.cpu().numpy(), np.zeros(hp, np.int32), cum, offsets_h, np.arange(hp) // 5, box[:hp], np.full(hp, tol))
    plain = verify_ref.counts(kept["vis"].view(np.uint64), depth.cpu().numpy(), np.zeros(hp, np.int32), None, None, None, box[:hp], np.full(hp, tol))
    same = (want[0].tobytes() == rows["masked"][0][:hp].cpu().numpy().tobytes() and plain[0].tobytes() == rows["counts"][0][:hp].cpu().numpy().tobytes()
            and not rows["masked"][1].any().item() and not rows["counts"][1].any().item())
    agree = rows["masked"][0][:, 2:4].sum().item() / max(1, rows["masked"][0][:, :8].sum().item())

    models = {1: dict(vertices=v, faces=f, diameter=diameter)}
    cameras = {(1, 1): dict(cam_K=K, depth=depth[0].cpu().numpy())}
    est = [dict(scene_id=1, im_id=1, obj_id=1, score=float(rs.uniform()), R=p[:3, :3].copy(), t=p[:3, 3].copy(), instance_id=i // 5) for i, p in enumerate(starts)]
    seg = dict(size=[H, W], counts=runs.tolist())
    segs = {d: seg for d in range(D)}
    verifier = verify.HypothesisVerifier(models, cameras)
    select = []
    for rep in range(1 + args.select_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chosen = verifier.select(est, segs)
        select.append((time.perf_counter() - t0) * 1e3)
    assert len(chosen) == D

    acc, cnt, msk = stats(times["accumulate"]), stats(times["counts"]), stats(times["masked"])
    spread = acc[2] - acc[1]
    held = cnt[0] <= acc[0] + spread
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each kernel call (its two memsets included), summed over the {len(chunks)} chunks of a "
             "repetition; times in ms: median (min .. max)",
             f"workload: {N} estimates of one object ({V} vertices, {F} faces, diameter {diameter:.1f}) on a {H} x {W} frame, {step} pairs per call; boxes hold "
             f"{box_pixels / N:.0f} pixels on average ({100.0 * box_pixels / (N * H * W):.1f}% of the frame); tol = gate = 0.05 diameters; {D} masks of {len(runs)} runs, "
             "one per 5 pairs", ""]
    for name, label in (("render", "render"), ("accumulate", "gpf_accumulate"), ("counts", "gpv_counts"), ("masked", "gpv_counts + masks")):
        m, lo, hi = stats(times[name])
        lines.append(f"   {label:<18}: {m:9.3f} ms ({lo:.3f} .. {hi:.3f})")
    lines += ["", f"condition: gpv_counts without masks {cnt[0]:.3f} ms <= gpf_accumulate {acc[0]:.3f} ms + its spread {spread:.3f} ms = {acc[0] + spread:.3f} ms: "
              f"{'HOLDS' if held else 'DOES NOT HOLD'}",
              f"gpv_counts: {box_pixels:.3e} box pixels, {12.0 * box_pixels / 1e9:.2f} GB of keys and depth -> {12.0 * box_pixels / (cnt[0] * 1e-3) / 1e9:.1f} GB/s without masks, "
              f"{12.0 * box_pixels / (msk[0] * 1e-3) / 1e9:.1f} GB/s with (a bisection of {len(runs)} prefix sums per box pixel); masks cost {msk[0] / cnt[0]:.2f}x",
              f"   the first {hp} pairs' counts, with and without masks, equal the restatement bit for bit and no status bit is set: {same}",
              f"   {100.0 * agree:.1f}% of the covered pixels agree with the depth within tol",
              f"HypothesisVerifier.select over {N} estimates of {D} detections (host work, uploads, render, counts, read-back; wall clock, {args.select_reps} runs after one): "
              f"median {np.median(select[1:]):.1f} ms (min {min(select[1:]):.1f}) = {1e3 * N / np.median(select[1:]):.0f} hypotheses per second"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not same:
        raise SystemExit("the device counts differ from the restatement")
    if not held:
        raise SystemExit("gpv_counts without masks is slower than gpf_accumulate by more than its spread")


if __name__ == "__main__":
    main()
