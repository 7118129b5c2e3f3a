"""Ingest measurement (needs one MI355X): frames + run-length masks -> crops against the dense-mask route on the same boxes.

Workload: 64 detections on eight 480 x 640 frames, masks = ellipses with a noisy rim, inputs in pinned host memory; 20
repetitions after 3 warm-ups, the two routes alternating inside every repetition, timed with HIP events.
  1. host to crops  : the host-to-device copies plus the kernels.  dense = frames + f32 masks (D,H,W) + boxes + ids, then
                      gp_preprocess_detections; rle = frames + ONE staging buffer (boxes, counts, offsets, ids), then
                      gpi_rle_scan + gpi_preprocess_detections_rle.  Bound: rle faster than dense.
  2. kernels alone  : inputs resident.  Bound: scan + fused kernel <= 2 x the dense kernel (guard against a pathological decoder).
  3. worst case     : one full-frame box on a 50 % random mask (~150 k runs: every pixel searches global memory).  No bound.
Writes the figures to --out (default profiles/ingest_rle.txt); exits 1 when a bound is missed."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import _lib, ingest  # noqa: E402
from gigapose_amd.crop import CLIP_MEAN, CLIP_STD  # noqa: E402
from gigapose_testing import synthetic as syn  # noqa: E402

DEV = "cuda"
T = 224
MEAN, STD = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)


def workload(seed=500, n_img=8, D=64, H=480, W=640):
    case = syn.detection_case(seed=seed, n_img=n_img, D=D, H=H, W=W)
    rs = np.random.RandomState(seed + 1)
    masks = case["masks"] != 0
    for d in range(D):   # noisy rim: 30 % of the pixels within 3 px of the outline flipped
        m = masks[d]
        rim = np.zeros_like(m)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                rim |= np.roll(np.roll(m, dy, 0), dx, 1) != m
        masks[d] = m ^ (rim & (rs.rand(H, W) < 0.3))
    case["masks"] = masks.astype(np.float32)
    return case


def dense_kernel(rgb, masks, boxes, im_id, out, err):
    n_img, _, H, W = rgb.shape
    _lib.call("gp_preprocess_detections", rgb, masks, boxes, im_id, n_img, masks.shape[0], H, W, T, MEAN, STD, out[0], out[1], out[2], err, _lib.stream_ptr())


def rle_kernels(rgb, counts, offsets, cum, boxes, im_id, out, err):
    n_img, _, H, W = rgb.shape
    D, total = offsets.numel() - 1, counts.numel()
    ingest._call("gpi_rle_scan", counts, offsets, total, D, H, W, cum, err, _lib.stream_ptr())
    ingest._call("gpi_preprocess_detections_rle", rgb, cum, offsets, total, boxes, im_id, n_img, D, H, W, T, MEAN, STD, out[0], out[1], out[2], err,
                 _lib.stream_ptr())


def outputs(D):
    return [torch.empty(D, 3, T, T, device=DEV), torch.empty(D, T, T, device=DEV), torch.empty(D, 3, 3, device=DEV)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def stats(v):
    v = np.sort(np.asarray(v))
    return f"median {np.median(v):9.1f} us   min {v[0]:9.1f}   max {v[-1]:9.1f}"


def measure(routes, reps, warmup):
    times = {k: [] for k in routes}
    for r in range(warmup + reps):
        for k, fn in routes.items():      # alternating: both routes see the same machine state
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_rle.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_ingest needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    case = workload()
    D, H, W = case["masks"].shape
    lists = [ingest.mask_to_rle_counts(m) for m in case["masks"]]
    counts, offsets = ingest.pack_rle([dict(counts=c, size=[H, W]) for c in lists], H, W)
    n_runs = np.diff(offsets)
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"workload: {D} detections on {case['rgb'].shape[0]} frames {H} x {W}, target {T}; ellipses with a noisy rim")
    say(f"runs per detection: min {n_runs.min()}  median {int(np.median(n_runs))}  max {n_runs.max()}  total {n_runs.sum()}")

    # pinned host inputs
    h_rgb = torch.from_numpy(case["rgb"]).pin_memory()
    h_masks = torch.from_numpy(case["masks"]).pin_memory()
    h_boxes = torch.from_numpy(case["boxes"]).pin_memory()
    h_im = torch.from_numpy(case["im_id"]).pin_memory()
    stage, spans = ingest.FrameIngest.stage(counts, offsets, case["boxes"], case["im_id"], np.zeros((0, 3, 3), np.float32))
    bytes_dense = h_rgb.numel() + 4 * h_masks.numel() + 8 * h_boxes.numel() + 4 * h_im.numel()
    bytes_rle = h_rgb.numel() + stage.numel()
    say(f"bytes copied host to device: dense {bytes_dense} (masks {4 * h_masks.numel()})   rle {bytes_rle} (staging buffer {stage.numel()}, "
        f"of it run lengths {4 * len(counts)})   mask bytes ratio 1 / {4 * h_masks.numel() / (4 * len(counts)):.0f}")
    out_d, out_r = outputs(D), outputs(D)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def part(dbuf, name, dtype):
        a, b, shape = spans[name]
        return dbuf[a:b].view(dtype).view(shape)

    def host_dense():
        rgb = h_rgb.to(DEV, non_blocking=True)
        masks = h_masks.to(DEV, non_blocking=True)
        boxes = h_boxes.to(DEV, non_blocking=True)
        im = h_im.to(DEV, non_blocking=True)
        dense_kernel(rgb, masks, boxes, im, out_d, err)

    def host_rle():
        rgb = h_rgb.to(DEV, non_blocking=True)
        dbuf = stage.to(DEV, non_blocking=True)
        c, o = part(dbuf, "counts", torch.int32), part(dbuf, "offsets", torch.int32)
        rle_kernels(rgb, c, o, torch.empty_like(c), part(dbuf, "boxes", torch.int64), part(dbuf, "im_id", torch.int32), out_r, err)

    t = measure({"dense": host_dense, "rle": host_rle}, args.reps, args.warmup)
    assert int(err.item()) == 0
    same = all(torch.equal(a, b) for a, b in zip(out_d, out_r))
    say()
    say(f"1. host to crops (copies + kernels), {args.reps} repetitions after {args.warmup} warm-ups, routes alternating")
    say(f"   dense : {stats(t['dense'])}")
    say(f"   rle   : {stats(t['rle'])}")
    ok1 = np.median(t["rle"]) < np.median(t["dense"])
    say(f"   rle / dense = {np.median(t['rle']) / np.median(t['dense']):.3f}   bound: rle faster than dense -> {'PASS' if ok1 else 'FAIL'}")
    say(f"   outputs of the two routes equal bit for bit: {same}")

    # kernels alone
    rgb, masks = h_rgb.to(DEV), h_masks.to(DEV)
    boxes, im = h_boxes.to(DEV), h_im.to(DEV)
    c, o = torch.from_numpy(counts).to(DEV), torch.from_numpy(offsets).to(DEV)
    cum = torch.empty_like(c)
    t = measure({"dense": lambda: dense_kernel(rgb, masks, boxes, im, out_d, err),
                 "rle": lambda: rle_kernels(rgb, c, o, cum, boxes, im, out_r, err),
                 "scan": lambda: ingest._call("gpi_rle_scan", c, o, c.numel(), D, H, W, cum, err, _lib.stream_ptr())}, args.reps, args.warmup)
    say()
    say("2. kernels alone (inputs resident)")
    say(f"   dense kernel           : {stats(t['dense'])}")
    say(f"   rle scan + fused kernel: {stats(t['rle'])}")
    say(f"   rle scan alone         : {stats(t['scan'])}")
    ratio = np.median(t["rle"]) / np.median(t["dense"])
    ok2 = ratio <= 2.0
    say(f"   rle / dense = {ratio:.3f}   bound: <= 2 x the dense kernel -> {'PASS' if ok2 else 'FAIL: the bound is missed'}")

    # worst case
    rs = np.random.RandomState(7)
    wm = (rs.rand(1, H, W) < 0.5).astype(np.float32)
    wc = ingest.mask_to_rle_counts(wm[0])
    wo = np.asarray([0, len(wc)], np.int32)
    d_wm, d_wc, d_wo = torch.from_numpy(wm).to(DEV), torch.from_numpy(wc).to(DEV), torch.from_numpy(wo).to(DEV)
    wbox = torch.tensor([[0, 0, W, H]], dtype=torch.int64, device=DEV)
    wim = torch.zeros(1, dtype=torch.int32, device=DEV)
    wcum = torch.empty_like(d_wc)
    o1d, o1r = outputs(1), outputs(1)
    t = measure({"dense": lambda: dense_kernel(rgb, d_wm, wbox, wim, o1d, err),
                 "rle": lambda: rle_kernels(rgb, d_wc, d_wo, wcum, wbox, wim, o1r, err)}, args.reps, args.warmup)
    assert int(err.item()) == 0 and all(torch.equal(a, b) for a, b in zip(o1d, o1r))
    say()
    say(f"3. worst case: one full-frame box on a 50 % random mask, {len(wc)} runs (searched in global memory); no bound")
    say(f"   dense kernel           : {stats(t['dense'])}")
    say(f"   rle scan + fused kernel: {stats(t['rle'])}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if (ok1 and ok2 and same) else 1


if __name__ == "__main__":
    sys.exit(main())
