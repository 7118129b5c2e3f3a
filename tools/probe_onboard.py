"""Onboarding measurement (needs one MI355X): the RGBA renders of ONE object -> template crops, stage by stage.

Workload: 162 renders at 480 x 640 (gigapose_testing.renders.object_renders) in pinned host memory, target 224; 20 repetitions
after 3 warm-ups, the stages alternating inside every repetition, timed with HIP events.
  upload  : the u8 renders host -> device (N*H*W*4 bytes)
  alpha   : gpo_alpha_boxes, a pure read of the same bytes (its three launches: init, the band kernel, finish)
  crop    : gpo_crop_templates; it writes N*(4*T*T + 9)*4 bytes and gathers one 4-byte pixel per output pixel inside the crop
  clone   : torch's copy of the same u8 buffer, the memory-rate yardstick: it moves TWICE the bytes the alpha pass reads
  host    : wall clock of the host route for the same object (numpy alpha boxes + oracle/crop_numpy.py + normalise), 16 threads
Bytes are computed from the shapes, rates follow from them.  Nothing here is a bound: the figures are recorded, not asserted
(the outputs are checked against the host route on the first 8 renders, and that check does fail the run).
Writes the figures to --out (default profiles/onboard_templates.txt)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import _lib, onboard  # noqa: E402
from gigapose_amd.crop import CLIP_MEAN, CLIP_STD  # noqa: E402
from gigapose_testing import renders  # noqa: E402

DEV = "cuda"
T = 224
MEAN, STD = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def measure(stages, reps, warmup):
    times = {k: [] for k in stages}
    for r in range(warmup + reps):
        for k, fn in stages.items():      # alternating: every stage sees the same machine state
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    return times


def line(name, v, nbytes, what):
    v = np.sort(np.asarray(v))
    med = float(np.median(v))
    return f"   {name:7s}: median {med:9.1f} us   min {v[0]:9.1f}   max {v[-1]:9.1f}   {nbytes / 1e6:8.1f} MB {what}   {nbytes / med / 1e3:8.1f} GB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onboard_templates.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--renders", type=int, default=162)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_onboard needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N, H, W = args.renders, 480, 640
    rgba = renders.object_renders(700, N, H, W)
    host = torch.from_numpy(rgba).pin_memory()
    dev = host.to(DEV)
    boxes = torch.empty(N, 4, dtype=torch.int64, device=DEV)
    out = [torch.empty(N, 3, T, T, device=DEV), torch.empty(N, T, T, device=DEV), torch.empty(N, 3, 3, device=DEV)]
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    in_bytes = N * H * W * 4
    out_bytes = N * (4 * T * T + 9) * 4
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"workload: one object, {N} renders {H} x {W} RGBA u8 in pinned host memory ({in_bytes / 1e6:.1f} MB), target {T}")

    def alpha():
        onboard._call("gpo_alpha_boxes", dev, N, H, W, boxes, err[0:1], _lib.stream_ptr())

    def crop():
        onboard._call("gpo_crop_templates", dev, boxes, N, H, W, T, MEAN, STD, out[0], out[1], out[2], err[1:2], _lib.stream_ptr())

    alpha()
    t = measure({"upload": lambda: host.to(DEV, non_blocking=True), "alpha": alpha, "crop": crop, "clone": lambda: dev.clone()},
                args.reps, args.warmup)
    assert err.tolist() == [0, 0]
    say()
    say(f"device stages, {args.reps} repetitions after {args.warmup} warm-ups, alternating, HIP events")
    say(line("upload", t["upload"], in_bytes, "copied "))
    say(line("alpha", t["alpha"], in_bytes, "read   "))
    say(line("crop", t["crop"], out_bytes, "written"))
    say(line("clone", t["clone"], 2 * in_bytes, "moved  "))
    ratio = np.median(t["alpha"]) / np.median(t["clone"])
    say(f"   alpha / clone = {ratio:.3f} in time; the clone moves twice the bytes, so at the clone's memory rate the alpha pass would take 0.500")
    say(f"   the renders ({in_bytes / 2 ** 20:.0f} MiB) fit the 256 MiB Infinity Cache and the device stages alternate over the same buffer: "
        "these are rates of the cache hierarchy, not of HBM alone")
    total = np.median(t["upload"]) + np.median(t["alpha"]) + np.median(t["crop"])
    say(f"   upload + alpha + crop = {total / 1e3:.2f} ms per object (sum of the medians)")

    torch.set_num_threads(16)
    n_chk = min(N, 8)
    t0 = time.perf_counter()
    ref = renders.prepare_numpy(rgba, target=T)
    host_s = time.perf_counter() - t0
    say()
    say(f"host route (numpy alpha boxes + oracle/crop_numpy.py + normalise, {torch.get_num_threads()} threads), the same object: "
        f"{host_s * 1e3:.0f} ms wall clock = {host_s * 1e6 / total:.0f} x the device route")
    same = bool((boxes.cpu().numpy() == ref[3]).all())
    for got, want in zip(out, ref[:3]):
        same &= got[:n_chk].cpu().numpy().tobytes() == want[:n_chk].tobytes()
    say(f"boxes of all {N} renders and the crops of the first {n_chk} equal the host route bit for bit: {same}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
