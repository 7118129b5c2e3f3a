"""Depth refinement measurement (needs one MI355X): the stages of DepthRefiner's loop at BOP-like sizes, beside the numpy
restatement on the host.

Workload (seeded, generated here): --pairs 1 500 estimates of one object (an icosphere(5)-sized mesh, 20 480 faces, pulled out
of round so that the rotation is constrained) on one 480 x 640 frame whose depth is the object at its true pose in front of a
wall; the estimates are the true pose moved by up to 4 degrees and 4 % of the diameter; boxes are the projected model's bounding
boxes padded by 8 pixels.  --iters 10 iterations, the pairs chunked as DepthRefiner chunks them (the keys of a call below 1 GiB).
HIP events are placed around the three stages of an iteration separately, summed over the chunks of every iteration: render
(render.project + render.raster), accumulate (gpf_accumulate with its two memsets), update (gpf_update); --reps repetitions
after --warmup warm-ups, every repetition from the same start poses.
accumulate's traffic is counted from the boxes: 8 bytes of key + 4 bytes of depth per box pixel (the normals, poses and sums
are a few kilobytes per pair and not counted); beside it, a device-to-device copy of 1 GiB (read + write counted).
The host column is gigapose_testing/refine_ref.py's accumulate on --host-pairs of the same keys, one thread, SCALED to all pairs
and iterations; the device sums of those pairs must equal it bit for bit, and the run fails otherwise.  Nothing here is a
bound: the figures are recorded.  Writes --out (default profiles/refine_depth.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import _lib, refine, render  # noqa: E402
from gigapose_testing import meshes, refine_ref  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_depth.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--level", type=int, default=5, help="subdivisions of the icosphere")
    ap.add_argument("--host-pairs", type=int, default=2)
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
    step = max(1, min(render.VIS_BYTES_PER_CALL // (H * W * 8), refine.MAX_PAIRS_PER_CALL))
    chunks = [(a, b) for _, a, b in _lib.chunked(N, step)]
    V, F = v.shape[0], f.shape[0]
    K9 = render._k9(K)
    buffers = render.KeyBuffers(min(N, step), V, F, H, W, DEV)
    start_d, Kd, boxd = dev(starts), dev(Kn), dev(box)
    frame = torch.zeros(N, dtype=torch.int32, device=DEV)
    gate, scale = torch.full((N,), 0.25 * diameter, dtype=torch.float64, device=DEV), torch.full((N,), diameter, dtype=torch.float64, device=DEV)
    sums, status = torch.empty(N, refine.SUMS, dtype=torch.int64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    clipped = torch.empty(N, dtype=torch.int32, device=DEV)
    t_render, t_acc, t_upd = Stage(), Stage(), Stage()
    kept = {}

    def run(iters, keep_first=False):
        poses, state = start_d.clone(), torch.zeros(N, dtype=torch.int32, device=DEV)
        poses32 = poses.to(torch.float32)
        for it in range(iters):
            for a, b in chunks:
                keys = t_render(lambda: buffers.draw(vd, fd, poses32[a:b], K9, 1e-3, clipped[a:b])[0])
                t_acc(lambda: refine.accumulate(keys, c, poses[a:b], Kd[a:b], depth, frame[a:b], boxd[a:b], gate[a:b], scale[a:b],
                                                out=(sums[a:b], status[a:b])))
                if keep_first and it == 0 and a == 0:
                    kept["vis"], kept["sums"], kept["status"] = keys[:args.host_pairs].cpu().numpy(), sums[:args.host_pairs].cpu().numpy(), status[:args.host_pairs].cpu().numpy()
                t_upd(lambda: refine.update(sums[a:b], clipped[a:b], scale[a:b], start_d[a:b], poses[a:b], poses32[a:b], state[a:b], min_points=32, min_pivot=1e-3,
                                            damping=0.0, tol2=1e-12))
        torch.cuda.synchronize()
        return poses, state

    times = {"render": [], "accumulate": [], "update": []}
    for rep in range(args.warmup + args.reps):
        poses, state = run(args.iters, keep_first=rep == 0)
        ms = (t_render.ms(), t_acc.ms(), t_upd.ms())
        if rep >= args.warmup:
            for k, t in zip(times, ms):
                times[k].append(t)
    buf = torch.empty(1 << 27, dtype=torch.int64, device=DEV)
    dst = torch.empty_like(buf)
    t_copy = Stage()
    copies = []
    for rep in range(args.warmup + args.reps):
        t_copy(lambda: dst.copy_(buf))
        torch.cuda.synchronize()
        copies.append(t_copy.ms())
    copy_ms = stats(copies[args.warmup:])[0]

    hp = args.host_pairs
    t0 = time.perf_counter()
    want = refine_ref.accumulate(kept["vis"].view(np.uint64), c.cpu().numpy(), starts[:hp], Kn[:hp], depth.cpu().numpy(), np.zeros(hp, np.int32), box[:hp],
                                 np.full(hp, 0.25 * diameter), np.full(hp, diameter))
    host_s = time.perf_counter() - t0
    same = want[0].tobytes() == kept["sums"].tobytes() and want[1].tobytes() == kept["status"].tobytes()
    poses_h, state_h = poses.cpu().numpy(), state.cpu().numpy()
    begin = np.asarray([cases.deviation(v, p, gt) for p in starts[:200]])
    end = np.asarray([cases.deviation(v, p, gt) for p in poses_h[:200]])

    acc = stats(times["accumulate"])
    calls = args.iters * len(chunks)
    bytes_acc = 12.0 * box_pixels * args.iters
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each stage, summed over the {len(chunks)} chunks x {args.iters} iterations of a "
             "repetition; times in ms: median (min .. max)",
             f"workload: {N} estimates of one object ({V} vertices, {F} faces, diameter {diameter:.1f}) on a {H} x {W} frame, {args.iters} iterations, "
             f"{step} pairs per call; boxes hold {box_pixels / N:.0f} pixels on average ({100.0 * box_pixels / (N * H * W):.1f}% of the frame)", ""]
    for name in ("render", "accumulate", "update"):
        m, lo, hi = stats(times[name])
        lines.append(f"   {name:<11}: {m:10.3f} ms ({lo:.3f} .. {hi:.3f})   {m / calls:8.3f} ms per call")
    total = sum(stats(times[k])[0] for k in times)
    lines += [f"   the three  : {total:10.3f} ms = {1e3 * N / total:.0f} estimates refined per second ({args.iters} iterations each)", "",
              f"accumulate: {box_pixels * args.iters:.3e} box pixel visits, {bytes_acc / 1e9:.2f} GB of keys and depth -> {bytes_acc / (acc[0] * 1e-3) / 1e9:.1f} GB/s; "
              f"a device-to-device copy of 1 GiB runs at {2.0 * buf.numel() * 8 / (copy_ms * 1e-3) / 1e9:.1f} GB/s (read + write)",
              f"   host   : {host_s / hp * N * args.iters * 1e3:10.1f} ms numpy restatement of accumulate, one thread, measured on {hp} of {N} pairs at the first iteration "
              f"and SCALED; device is {host_s / hp * N * args.iters * 1e3 / acc[0]:.0f}x",
              f"   the first {hp} pairs' sums and status at the first iteration equal the restatement bit for bit: {same}",
              f"   state after {args.iters} iterations: {int((state_h & refine.STOP == 0).sum())} of {N} pairs not stopped, {int((state_h & refine.CONVERGED != 0).sum())} converged; "
              f"largest vertex deviation of the first 200: start median {np.median(begin):.3f} max {begin.max():.3f} -> end median {np.median(end):.4f} max {end.max():.4f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not same:
        raise SystemExit("the device sums differ from the restatement")


if __name__ == "__main__":
    main()
