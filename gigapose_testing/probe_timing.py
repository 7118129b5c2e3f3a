"""What the renderers' measurement tools (tools/probe_render.py, probe_texture.py, probe_shade.py) share: HIP-event timing of
stages that alternate inside every repetition, the line a stage is reported with and the commit a figure is recorded under."""
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def line(name, v, what, width=12):
    v = np.sort(np.asarray(v))
    return f"   {name:{width}s}: median {float(np.median(v)):9.1f} us   min {v[0]:9.1f}   max {v[-1]:9.1f}   {what}"


def commit():
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    return (r.stdout.strip() + (" + uncommitted changes" if dirty else "")) if r.returncode == 0 else "unknown (no git here)"
