"""Ground-truth visibility measurement (needs one MI355X): gpg_classify, the two run kernels and the drawing, at the shape of
profiles/verify_hypotheses.txt, on the canvas of margin 1.0 and of margin 0; and a whole GroundTruthInfo.compute.

Workload (seeded, generated here; tools/probe_verify.py's object): --instances 1 500 ground truths of one object (an
icosphere(5)-sized mesh, 20 480 faces) on one 480 x 640 frame whose depth is the object at a central pose in front of a wall; the
ground truths are that pose turned by up to 30 degrees and moved by up to 1.5 diameters sideways and 0.5 in depth, so that some are
hidden by the central one and some leave the frame; the views chunked as evaluate.vsd_errors chunks them (the keys of a call below
1 GiB: 48 views of the 1440 x 1920 canvas, 436 of the frame).  Per repetition every chunk is drawn once and the three kernels run on
it with HIP events around each call (its memsets and its initialising launch included), summed over the chunks; the run kernels
encode the visible bit, with the lists sized once before the timed repetitions.  --reps repetitions after --warmup warm-ups.

No time is required of this stage: there is no earlier code to compare with.  The run fails if the rows, class bytes or lists of
the first --host-instances instances differ from the numpy restatement.  Writes --out (default profiles/gtinfo_visibility.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import _lib, evaluate, gtinfo, render  # noqa: E402
from gigapose_testing import gtinfo_ref, meshes  # noqa: E402
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


def kernels(args, margin, vd, fd, poses32, depth, ray, v, f):
    """-> the lines of one margin, and whether the first instances equal the restatement."""
    N = len(poses32)
    Hc, Wc, ox, oy = gtinfo.canvas(H, W, margin)
    Kc = K.copy()
    Kc[2], Kc[5] = Kc[2] + ox, Kc[5] + oy
    K9 = render._k9(Kc)
    step = render.views_step(None, Hc, Wc)
    chunks = [(a, b) for _, a, b in _lib.chunked(N, step)]
    buffers = render.KeyBuffers(min(N, step), v.shape[0], f.shape[0], Hc, Wc, DEV)
    clipped = torch.empty(N, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(N, dtype=torch.int32, device=DEV)
    stages = {k: Stage() for k in ("render", "classify", "count_runs", "write_runs")}
    sized, kept = {}, {}

    def run(rep):
        for a, b in chunks:
            keys = stages["render"](lambda: buffers.draw(vd, fd, poses32[a:b], K9, 1e-3, clipped[a:b])[0])
            cls, info, box, status = stages["classify"](lambda: gtinfo.classify(keys, (ox, oy), depth, zeros[a:b], ray, zeros[a:b], args.delta))
            runs, work = stages["count_runs"](lambda: gtinfo.count_runs(cls, 1))
            if a not in sized:                                      # once, outside the timed repetitions: the lists' sizes
                offsets = torch.zeros(b - a + 1, dtype=torch.int64, device=DEV)
                offsets[1:] = torch.cumsum(runs, 0)
                total = int(offsets[-1])
                sized[a] = (offsets.to(torch.int32), torch.empty(total, dtype=torch.int32, device=DEV), torch.empty(total, dtype=torch.int32, device=DEV),
                            torch.zeros(1, dtype=torch.int32, device=DEV))
            offsets, counts, cum, err = sized[a]
            stages["write_runs"](lambda: gtinfo.write_runs(cls, 1, work, offsets, (counts, cum), err))
            if rep == 0 and a == 0:
                hp = args.host_instances
                kept.update(vis=keys[:hp].cpu().numpy(), cls=cls[:hp].cpu().numpy(), info=info[:hp].cpu().numpy(), box=box[:hp].cpu().numpy(),
                            counts=counts[:int(offsets[hp])].cpu().numpy(), cum=cum[:int(offsets[hp])].cpu().numpy(), err=int(err.item()))
            if rep == 0:
                kept.setdefault("info_all", []).append(info.cpu().numpy())
                kept.setdefault("runs_all", []).append(runs.cpu().numpy())
        torch.cuda.synchronize()

    times = {k: [] for k in stages}
    for rep in range(args.warmup + args.reps):
        run(rep)
        for k in stages:
            t = stages[k].ms()
            if rep >= args.warmup:
                times[k].append(t)
    hp = args.host_instances
    want = gtinfo_ref.classify(kept["vis"].view(np.uint64), (ox, oy), depth.cpu().numpy(), np.zeros(hp, np.int32), ray.cpu().numpy(), np.zeros(hp, np.int32), args.delta)
    lists = gtinfo_ref.encode_runs(want[0], 1)
    same = (all(kept[k].tobytes() == w.tobytes() for k, w in zip(("cls", "info", "box"), want)) and kept["counts"].tobytes() == lists[0].tobytes()
            and kept["cum"].tobytes() == lists[1].tobytes() and kept["err"] == 0 and not clipped.any().item())
    info = np.concatenate(kept["info_all"])
    fract = info[:, gtinfo.PX_VISIB] / np.maximum(info[:, gtinfo.PX_ALL], 1)
    key_bytes, cls_bytes = 8.0 * N * Hc * Wc, 1.0 * N * H * W
    cl = stats(times["classify"])
    lines = [f"margin {margin}: canvas {Hc} x {Wc}, origin ({ox}, {oy}), {step} views per call, {len(chunks)} calls per repetition",
             f"   object pixels per instance: {info[:, gtinfo.PX_ALL].mean():.0f} on the canvas, {info[:, gtinfo.PX_FRAME].mean():.0f} in the frame; visib_fract: mean "
             f"{fract.mean():.3f}, {int((fract < 0.1).sum())} of {N} below 0.1, {int((fract == 1).sum())} equal to 1; runs of the visible mask per instance: "
             f"{np.concatenate(kept['runs_all']).mean():.0f}"]
    for name, label in (("render", "drawing"), ("classify", "gpg_classify"), ("count_runs", "gpg_count_runs"), ("write_runs", "gpg_write_runs")):
        m, lo, hi = stats(times[name])
        lines.append(f"   {label:<16}: {m:9.3f} ms ({lo:.3f} .. {hi:.3f})")
    lines += [f"   gpg_classify reads {key_bytes / 1e9:.2f} GB of keys and writes {cls_bytes / 1e9:.2f} GB of class bytes (zeroed first): "
              f"{(key_bytes + 2 * cls_bytes) / (cl[0] * 1e-3) / 1e9:.0f} GB/s",
              f"   the first {hp} instances' rows, class bytes and lists equal the restatement bit for bit, no list is refused and no view is clipped: {same}", ""]
    return lines, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtinfo_visibility.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--instances", type=int, default=1500)
    ap.add_argument("--level", type=int, default=5, help="subdivisions of the icosphere")
    ap.add_argument("--host-instances", type=int, default=2)
    ap.add_argument("--compute-reps", type=int, default=3)
    ap.add_argument("--delta", type=float, default=15.0)
    args = ap.parse_args()
    rs = np.random.RandomState(7)
    v, f, _ = meshes.icosphere(args.level, 1.0)
    v = (v.astype(np.float64) * (60.0, 45.0, 30.0) * (1.0 + 0.15 * np.sin(4.0 * v[:, [1, 2, 0]]))).astype(np.float32)
    diameter = float(2 * np.linalg.norm(v, axis=1).max())
    centre = cases.rigid(cases.rot([1, 2, 3], 35), (30.0, -20.0, 600.0))
    N = args.instances
    poses = np.stack([cases.moved(centre, rs.standard_normal(3), rs.uniform(0, 30), rs.uniform(-1, 1, 3) * (1.5, 1.5, 0.5) * diameter) for _ in range(N)])
    vd, fd = dev(v), dev(f)
    truth = render.MeshRenderer(H, W, K)(vd, fd, None, dev(centre[None].astype(np.float32)), colour=(255, 255, 255))["depth"]
    depth = torch.round(torch.where(truth > 0, truth, torch.full_like(truth, 900.0)))
    ray = dev(evaluate.ray_map(K, H, W)[None])
    poses32 = dev(poses.astype(np.float32))
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each call (memsets and the initialising launch included), summed over the calls of a "
             "repetition; times in ms: median (min .. max)",
             f"workload: {N} ground truths of one object ({v.shape[0]} vertices, {f.shape[0]} faces, diameter {diameter:.1f}) on a {H} x {W} frame; delta = {args.delta}; "
             "the run kernels encode the visible bit", ""]
    ok = True
    for margin in (1.0, 0.0):
        part, same = kernels(args, margin, vd, fd, poses32, depth, ray, v, f)
        lines += part
        ok = ok and same
    models = {1: dict(vertices=v, faces=f, diameter=diameter)}
    cameras = {(1, 1): dict(cam_K=K, depth=depth[0].cpu().numpy())}
    gts = {(1, 1): [dict(obj_id=1, cam_R_m2c=p[:3, :3].reshape(9).tolist(), cam_t_m2c=p[:3, 3].tolist()) for p in poses]}
    for masks in (False, True):
        g = gtinfo.GroundTruthInfo(models, cameras, delta=args.delta, margin=1.0)
        wall = []
        for rep in range(1 + args.compute_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = g.compute(gts, masks=masks)
            wall.append((time.perf_counter() - t0) * 1e3)
        assert len(out[(1, 1)]) == N
        lines.append(f"GroundTruthInfo.compute at margin 1.0, masks={masks} (host work, uploads, drawing, kernels, read-back; wall clock, {args.compute_reps} runs after one): "
                     f"median {np.median(wall[1:]):.1f} ms (min {min(wall[1:]):.1f}) = {1e3 * N / np.median(wall[1:]):.0f} ground truths per second")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not ok:
        raise SystemExit("the device results differ from the restatement")


if __name__ == "__main__":
    main()
