"""All-pairs distance measurement (needs one MI355X): the entry points of libgigapose_dist.so at T-LESS-like sizes, beside the numpy
restatement on the host.

Workloads (seeded, generated here):
  ADD-S     : 1 500 (estimate, ground truth) pairs x 5 000 vertices: 3.75e10 point pairs
  ADD       : the same pairs and vertices
  diameter  : V = 5 000 and V = 50 000
Each is timed with HIP events around the whole entry point (its memsets and its launch), --reps repetitions after --warmup
warm-ups, the workloads alternating inside every repetition.  Operations are counted from the shapes by the code below:
  ADD-S     : 9 float64 operations per point pair (3 differences, 3 products, 2 sums, 1 minimum) + 36 per (pair, vertex) for the
              two transforms; the transforms a workgroup repeats while it stages the estimate's points (ceil(V / 1024) times) and
              the root are not counted
  ADD       : 36 + 8 per (pair, vertex); it is bound by launch and memory, not by arithmetic: pairs per second are what matters
  diameter  : 9 per pair i < j (the kernel also visits the lower half of the tiles on the diagonal; not counted)
The arithmetic contract forbids fusing a product with a sum, so the ceiling for these kernels is HALF the float64 vector rate,
which counts a fused multiply-add as two.  That rate is the MI355X data sheet's 78.6 TFLOP/s (256 compute units x 128 FLOP per
clock x 2.4 GHz); nothing in this repository has measured it, and the clock under load is lower.
The host column is gigapose_testing/dist_ref.py on a stated FRACTION of the same inputs, scaled (the diameter at V = 50 000 is
scaled from V = 5 000 by the number of pairs); the device result of that fraction must equal it bit for bit, and the run fails
otherwise.  numpy's element-wise loops use one thread.  Nothing here is a bound: the figures are recorded.
Writes --out (default profiles/dist_errors.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import distances  # noqa: E402
from gigapose_testing import dist_ref, eval_cases  # noqa: E402

DEV = "cuda"
F64_VECTOR_PEAK = 78.6e12          # FLOP/s: the MI355X data sheet's float64 vector rate (an FMA = 2)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3   # s


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stats(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[0]), float(v[-1])


def key_value(t):
    return int(t.cpu().numpy().view(np.uint64)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_errors.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--vertices", type=int, default=5000)
    ap.add_argument("--big", type=int, default=50000, help="vertices of the large diameter")
    ap.add_argument("--host-pairs", type=int, nargs=2, default=[2, 150], help="pairs the host restatement computes: ADD-S, ADD")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_dist needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N, V = args.pairs, args.vertices
    rs = np.random.RandomState(1)
    vertices = rs.uniform(-60, 60, (V, 3)).astype(np.float32)
    big = rs.uniform(-60, 60, (args.big, 3)).astype(np.float32)
    gt = np.stack([eval_cases.rigid(eval_cases.rotation(rs), (rs.uniform(-80, 80), rs.uniform(-60, 60), rs.uniform(400, 900))) for _ in range(N)])
    est = np.stack([g @ eval_cases.small_motion(rs, 0.05, 3.0) for g in gt])
    d_v, d_big, d_est, d_gt = dev(vertices), dev(big), dev(est), dev(gt)

    stages = {"adds": lambda: distances.add_sums(d_v, d_est, d_gt, True), "add": lambda: distances.add_sums(d_v, d_est, d_gt, False),
              "diameter": lambda: distances.diameter2_key(d_v), "diameter_big": lambda: distances.diameter2_key(d_big)}
    times = {k: [] for k in stages}
    for r in range(args.warmup + args.reps):
        for k, fn in stages.items():
            t = timed(fn)
            if r >= args.warmup:
                times[k].append(t)

    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"{args.reps} repetitions after {args.warmup} warm-ups, workloads alternating, HIP events around the whole entry point; times in ms: median (min .. max)")
    say(f"float64 vector peak {F64_VECTOR_PEAK / 1e12:.1f} TFLOP/s: the data sheet's figure (256 CUs x 128 FLOP/clock x 2.4 GHz), not measured here; it counts "
        f"an FMA as two, so -ffp-contract=off kernels can reach half of it ({F64_VECTOR_PEAK / 2e12:.1f})")
    ok = True
    for name, symmetric, hp in (("adds", True, args.host_pairs[0]), ("add", False, args.host_pairs[1])):
        hp = min(hp, N)
        t0 = time.perf_counter()
        want = dist_ref.add_sums(vertices, est[:hp], gt[:hp], symmetric)
        host = (time.perf_counter() - t0) * N / hp
        got = stages[name]()
        same = all(g[:hp].cpu().numpy().tobytes() == x.tobytes() for g, x in zip(got, want))
        clean = not bool(got[1].any().item())
        ok &= same and clean
        med, lo, hi = stats(times[name])
        ops = (9 * N * V * V + 36 * N * V) if symmetric else 44 * N * V
        say()
        say(f"gpd_{name}: N {N}, V {V}: " + (f"{N * V * V:.3e} point pairs, " if symmetric else f"{N * V:.3e} points, ") + f"{ops:.3e} float64 operations")
        rate = (f"{ops / med / 1e12:6.2f} TFLOP/s achieved = {100 * ops / med / (F64_VECTOR_PEAK / 2):.1f}% of the unfused ceiling, "
                f"{100 * ops / med / F64_VECTOR_PEAK:.1f}% of the vector peak (compute bound)") if symmetric else \
            f"{N / med / 1e6:.2f} M pairs/s, {ops / med / 1e12:.3f} TFLOP/s ({12 * V * 1e-3:.0f} KB of vertices re-read per pair from cache: launch and memory bound)"
        say(f"   device : {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})   {rate}")
        say(f"   host   : {host * 1e3:9.1f} ms numpy restatement, one thread, measured on {hp} of {N} pairs and SCALED; device is {host / med:.0f}x")
        say(f"   the first {hp} pairs equal the restatement bit for bit (sums and status): {same}; no status bit set: {clean}; "
            f"mean error of pair 0: {distances.errors_from_sums(got[0][:1].cpu().numpy(), got[1][:1].cpu().numpy(), V, 20)[0]:.6f}")
    t0 = time.perf_counter()
    want = dist_ref.diameter2_key(vertices)
    host = time.perf_counter() - t0
    for name, verts, n, scaled in (("diameter", vertices, V, False), ("diameter_big", big, args.big, True)):
        got = key_value(stages[name]())
        med, lo, hi = stats(times[name])
        pairs = n * (n - 1) // 2
        ops = 9 * pairs
        h = host * pairs / (V * (V - 1) // 2)
        say()
        say(f"gpd_diameter2: V {n}: {pairs:.3e} pairs, {ops:.3e} float64 operations")
        say(f"   device : {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})   {ops / med / 1e12:6.2f} TFLOP/s achieved = "
            f"{100 * ops / med / (F64_VECTOR_PEAK / 2):.1f}% of the unfused ceiling ({(n + 1023) // 1024 * ((n + 1023) // 1024 + 1) // 2} workgroups of work on 256 compute units)")
        say(f"   host   : {h * 1e3:9.1f} ms numpy restatement, one thread" + (f", SCALED from V = {V} by the number of pairs" if scaled else ", measured")
            + f"; device is {h / med:.0f}x")
        if not scaled:
            same = got == want
            ok &= same
            say(f"   the key equals the restatement's: {same}; diameter {np.sqrt(np.asarray([got], np.uint64).view(np.float64))[0]:.6f}")
        else:
            v64 = verts.astype(np.float64)                       # a check that finishes: the farthest pair among the 512 vertices farthest from the centroid
            far = v64[np.argsort(((v64 - v64.mean(axis=0)) ** 2).sum(axis=1))[-512:]]
            lower = float(np.asarray([dist_ref.diameter2_key(far.astype(np.float32))], np.uint64).view(np.float64)[0])
            value = float(np.asarray([got], np.uint64).view(np.float64)[0])
            sane = lower <= value <= 3 * 120.0 ** 2
            ok &= sane
            say(f"   diameter {np.sqrt(value):.6f}; at least the farthest pair among the 512 outermost vertices ({np.sqrt(lower):.6f}) and at most the box diagonal: {sane}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
