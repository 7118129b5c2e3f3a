"""Pose-scoring measurement (needs one MI355X): the two entry points of libgigapose_eval.so at T-LESS-like sizes, beside the numpy
restatement on the host.

Workloads (seeded, generated here):
  mssd/mspd A : 1 500 (estimate, ground truth) pairs x 5 000 vertices x 2 symmetry transforms      (an object with one half turn)
  mssd/mspd B : 1 500 pairs x 10 000 vertices x 630 transforms                                      (a half turn x a discretised axis)
  vsd         : 1 500 pairs of 480 x 640 depth maps, 10 thresholds, 50 sensor frames, one ray map
Each is timed with HIP events around the whole entry point (its memset and every launch), --reps repetitions after --warmup
warm-ups, the workloads alternating inside every repetition.  Operations and bytes are counted from the shapes by the code below:
  mssd/mspd : 43 float64 operations per (pair, symmetry, vertex) -- 18 for the ground truth's transform, 3 + 5 for d2, 12 for its
              projection (two of them divisions, counted as one each), 2 + 3 for p2 -- plus 30 per (pair, vertex) for the estimate (transform and projection);
              the arithmetic contract forbids fusing a product with a sum, so the ceiling for these kernels is HALF the float64
              vector rate, which counts a fused multiply-add as two
  vsd       : 20 bytes requested per (pair, pixel): 4 + 4 of the two renders (read once from HBM), 4 of the sensor frame and 8 of
              the ray map (shared by many pairs: mostly cache hits), so both the requested and the HBM bytes are given
The host column is gigapose_testing/eval_ref.py on a stated FRACTION of the same inputs, scaled; the device result of that
fraction must equal it bit for bit, and the run fails otherwise.  numpy's element-wise loops use one thread: the 16-thread figure
is that time / 16, the best a perfect split could do, and is labelled as such.  Nothing here is a bound: the figures are recorded.
Writes --out (default profiles/eval_scores.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import evaluate  # noqa: E402
from gigapose_testing import eval_cases, eval_ref  # noqa: E402

DEV = "cuda"
H, W = 480, 640
F64_VECTOR_PEAK = 78.6e12          # FLOP/s: the MI355X data sheet's float64 vector rate (an FMA = 2), half its 157.3 of float32
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12
OPS_PER_POINT, OPS_PER_EST_POINT = 43, 30


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3   # s


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pose_workload(seed, N, V, syms):
    vertices, est, gt, K = eval_cases.pose_case(seed, V, N, syms)
    t = dict(vertices=dev(vertices), syms=dev(syms), est=dev(est), gt=dev(gt), K=dev(K))
    t["work"] = torch.empty(evaluate.pose_workspace_bytes(N, len(syms)) // 8, dtype=torch.int64, device=DEV)
    return dict(host=(vertices, syms, est, gt, K), dev=t, N=N, V=V, S=len(syms))


def vsd_workload(seed, N, M, T):
    """Depth maps made on the device: a disc of depth ~600 +- 40 per view on an empty frame, a sensor frame of ~640 with holes."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")

    def discs(n, base):
        cx = torch.rand(n, 1, 1, device=DEV, generator=g) * 300 + 170
        cy = torch.rand(n, 1, 1, device=DEV, generator=g) * 200 + 140
        inside = (xx[None] - cx) ** 2 + (yy[None] - cy) ** 2 < 110 ** 2
        d = base + torch.rand(n, H, W, device=DEV, generator=g) * 80
        return torch.where(inside, d, torch.zeros_like(d)).to(torch.float32).contiguous()

    de, dg = discs(N, 560.0), discs(N, 560.0)
    dt = (600.0 + torch.rand(M, H, W, device=DEV, generator=g) * 80).to(torch.float32)
    dt[torch.rand(M, H, W, device=DEV, generator=g) < 0.1] = 0.0
    frame = np.arange(N, dtype=np.int32) % M
    ray = dev(evaluate.ray_map(eval_cases.K_CAMERA, H, W)[None])
    thr = dev(np.tile(np.asarray(evaluate.TAUS) * 140.0, (N, 1)))
    return dict(de=de, dg=dg, dt=dt.contiguous(), frame=frame, ray=ray, ray_index=np.zeros(N, np.int32), thr=thr, N=N, M=M, T=T)


def stats(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[0]), float(v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_scores.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--host-pairs", type=int, nargs=3, default=[150, 2, 15], help="pairs the host restatement computes: A, B, vsd")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_eval needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N = args.pairs
    syms_b = evaluate.symmetry_transforms(eval_cases.CYLINDER)
    syms_a = evaluate.symmetry_transforms({"symmetries_discrete": [eval_cases.HALF_TURN_X]})
    A, B = pose_workload(1, N, 5000, syms_a), pose_workload(2, N, 10000, syms_b)
    Vs = vsd_workload(3, N, 50, 10)

    def run_pose(w):
        t = w["dev"]
        return evaluate.mssd_mspd(t["vertices"], t["syms"], t["est"], t["gt"], t["K"], 0.0, workspace=t["work"])

    def run_vsd(n=None):
        n = Vs["N"] if n is None else n
        return evaluate.vsd_counts(Vs["de"][:n], Vs["dg"][:n], Vs["dt"], Vs["frame"][:n], Vs["ray"], Vs["ray_index"][:n], 15.0, Vs["thr"][:n])

    stages = {"A": lambda: run_pose(A), "B": lambda: run_pose(B), "vsd": run_vsd}
    times = {k: [] for k in stages}
    for r in range(args.warmup + args.reps):
        for k, fn in stages.items():
            t = timed(fn)
            if r >= args.warmup:
                times[k].append(t)

    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"{args.reps} repetitions after {args.warmup} warm-ups, workloads alternating, HIP events around the whole entry point; times in ms: median (min .. max)")
    say(f"float64 vector peak {F64_VECTOR_PEAK / 1e12:.1f} TFLOP/s counts an FMA as two; -ffp-contract=off kernels can reach half of it "
        f"({F64_VECTOR_PEAK / 2e12:.1f}); HBM {HBM_PEAK / 1e12:.1f} TB/s spec, {HBM_MEASURED / 1e12:.2f} TB/s measured copy")
    ok = True
    host = {}
    for name, w, hp in (("A", A, args.host_pairs[0]), ("B", B, args.host_pairs[1])):
        hp = min(hp, N)
        vertices, syms, est, gt, K = w["host"]
        t0 = time.perf_counter()
        want = eval_ref.mssd_mspd2(vertices, syms, est[:hp], gt[:hp], K[:hp])
        host[name] = (time.perf_counter() - t0) * N / hp
        got = run_pose(w)
        same = all(g[:hp].cpu().numpy().tobytes() == x.tobytes() for g, x in zip(got, want))
        ok &= same
        med, lo, hi = stats(times[name])
        ops = OPS_PER_POINT * N * w["S"] * w["V"] + OPS_PER_EST_POINT * N * w["V"]
        say()
        say(f"gpe_mssd_mspd {name}: N {N}, V {w['V']}, S {w['S']}: {N * w['S'] * w['V']:.3e} point transforms, {ops:.3e} float64 operations")
        say(f"   device : {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})   {ops / med / 1e12:6.2f} TFLOP/s achieved = "
            f"{100 * ops / med / (F64_VECTOR_PEAK / 2):.1f}% of the unfused ceiling, {100 * ops / med / F64_VECTOR_PEAK:.1f}% of the vector peak (compute bound: "
            f"{(12 * w['V'] + 14 * 8 * w['S'] * 3) * N / 1e6:.0f} MB touched)")
        say(f"   host   : {host[name] * 1e3:9.1f} ms numpy restatement, one thread, measured on {hp} of {N} pairs and scaled; / 16 = "
            f"{host[name] / 16 * 1e3:.1f} ms if 16 threads split it perfectly; device is {host[name] / med:.0f}x (one thread), {host[name] / 16 / med:.0f}x (ideal 16)")
        say(f"   the first {hp} pairs equal the restatement bit for bit: {same}")
    hp = min(args.host_pairs[2], N)
    t0 = time.perf_counter()
    want = eval_ref.vsd_counts(Vs["de"][:hp].cpu().numpy(), Vs["dg"][:hp].cpu().numpy(), Vs["dt"].cpu().numpy(), Vs["frame"][:hp],
                               Vs["ray"].cpu().numpy(), Vs["ray_index"][:hp], 15.0, Vs["thr"][:hp].cpu().numpy())
    host["vsd"] = (time.perf_counter() - t0) * N / hp
    same = bool((run_vsd()[:hp].cpu().numpy() == want).all())
    ok &= same
    med, lo, hi = stats(times["vsd"])
    requested = N * H * W * 20
    hbm = N * H * W * 8 + Vs["M"] * H * W * 4 + H * W * 8
    say()
    say(f"gpe_vsd_counts: N {N}, {H} x {W}, T {Vs['T']}, M {Vs['M']} frames, one ray map: {N * H * W:.3e} pixels")
    say(f"   device : {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})   {requested / med / 1e12:5.2f} TB/s requested (20 B per pixel), "
        f"{hbm / med / 1e12:5.2f} TB/s of bytes that must come from HBM ({hbm / 1e9:.2f} GB: the two renders once, frames and ray map once) = "
        f"{100 * hbm / med / HBM_PEAK:.1f}% of spec, {100 * hbm / med / HBM_MEASURED:.1f}% of the measured copy rate (memory bound)")
    say(f"   host   : {host['vsd'] * 1e3:9.1f} ms numpy restatement, one thread, measured on {hp} of {N} pairs and scaled; / 16 = "
        f"{host['vsd'] / 16 * 1e3:.1f} ms; device is {host['vsd'] / med:.0f}x (one thread), {host['vsd'] / 16 / med:.0f}x (ideal 16)")
    say(f"   the first {hp} pairs equal the restatement exactly: {same}; union of pair 0 {int(want[0, 0])}, intersection {int(want[0, 1])}, bad {want[0, 2:].tolist()}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
