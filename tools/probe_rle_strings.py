"""Compressed run-length strings measurement (needs one MI355X): the string route (bytes to the GPU, gps_rle_string_scan) against
the list route (int32 run lengths to the GPU, gpi_rle_scan) on the workload and with the method of tools/probe_ingest.py.

Workload: 64 detections on eight 480 x 640 frames, masks = ellipses with a noisy rim, inputs in pinned host memory; 20 repetitions
after 3 warm-ups, the routes alternating inside every repetition, timed with HIP events.
  1. bytes shipped   : the staging buffer of each route and its mask part.  Expectation: the mask part shrinks 2 - 4 x.
  2. host to crops   : the host-to-device copies plus the kernels (scan + gpi_preprocess_detections_rle), both routes.
  3. scans alone     : gps_rle_string_scan against gpi_rle_scan, inputs resident.  Expectation: within 2 x (two passes against one).
  4. one noise mask  : the same two scans on one 50 % random mask (~150 k runs in one workgroup).  No expectation.
  5. host cost today : what a user without this route pays on the CPU -- a sequential Python decode of the same strings, then
                       pack_rle -- and the vectorised numpy decoder next to it.  Wall clock, one pass.
Recorded, not gating: writes the figures to --out (default profiles/ingest_rle_strings.txt); exits 1 only when the two routes'
outputs differ."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gigapose_amd import _lib, ingest  # noqa: E402
from gigapose_amd import rle_strings as rs  # noqa: E402
from gigapose_testing import rle_string_ref as ref  # noqa: E402
from probe_ingest import DEV, MEAN, STD, T, measure, outputs, rle_kernels, stats, workload  # noqa: E402


def string_scan(data, byte_offsets, offsets, counts, cum, H, W, err):
    rs._call("gps_rle_string_scan", data, byte_offsets, data.numel(), offsets, counts.numel(), offsets.numel() - 1, H, W, counts, cum, err, _lib.stream_ptr())


def list_scan(counts, offsets, cum, H, W, err):
    ingest._call("gpi_rle_scan", counts, offsets, counts.numel(), offsets.numel() - 1, H, W, cum, err, _lib.stream_ptr())


def string_kernels(rgb, data, byte_offsets, counts, offsets, cum, boxes, im_id, out, err):
    n_img, _, H, W = rgb.shape
    D = offsets.numel() - 1
    string_scan(data, byte_offsets, offsets, counts, cum, H, W, err)
    ingest._call("gpi_preprocess_detections_rle", rgb, cum, offsets, counts.numel(), boxes, im_id, n_img, D, H, W, T, MEAN, STD, out[0], out[1], out[2], err,
                 _lib.stream_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_rle_strings.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_rle_strings needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    case = workload()
    D, H, W = case["masks"].shape
    lists = [ingest.mask_to_rle_counts(m) for m in case["masks"]]
    strings = [rs.rle_string_from_counts(c) for c in lists]
    counts, offsets = ingest.pack_rle([dict(counts=c, size=[H, W]) for c in lists], H, W)
    data, byte_offsets, zero_counts, s_offsets = rs.pack_rle_any([dict(counts=s, size=[H, W]) for s in strings], H, W)
    assert (s_offsets == offsets).all()
    n_runs = np.diff(offsets)
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"workload: {D} detections on {case['rgb'].shape[0]} frames {H} x {W}, target {T}; ellipses with a noisy rim")
    say(f"runs per detection: min {n_runs.min()}  median {int(np.median(n_runs))}  max {n_runs.max()}  total {n_runs.sum()}")
    say(f"string bytes per run: {len(data) / len(counts):.2f}")

    h_rgb = torch.from_numpy(case["rgb"]).pin_memory()
    no_K = np.zeros((0, 3, 3), np.float32)
    stage_l, spans_l = ingest.FrameIngest.stage(counts, offsets, case["boxes"], case["im_id"], no_K)
    stage_s, spans_s, device_bytes = rs.CocoFrameIngest.stage(data, byte_offsets, zero_counts, s_offsets, case["boxes"], case["im_id"], no_K)
    say()
    say("1. bytes shipped host to device (next to the frames, the same for both routes: %d)" % h_rgb.numel())
    say(f"   list route  : staging buffer {stage_l.numel()}, of it run lengths {4 * len(counts)}")
    say(f"   string route: staging buffer {stage_s.numel()}, of it string bytes {len(data)} + byte offsets {4 * len(byte_offsets)} "
        f"(the list slots the kernel fills stay on the device: {4 * len(zero_counts)})")
    say(f"   mask part as coded: string / list = 1 / {4 * len(counts) / len(data):.2f}   staging buffer: string / list = "
        f"{stage_s.numel() / stage_l.numel():.3f}")
    out_l, out_s = outputs(D), outputs(D)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def part(dbuf, spans, name, dtype):
        a, b, shape = spans[name]
        return dbuf[a:b].view(dtype).view(shape)

    def host_list():
        rgb = h_rgb.to(DEV, non_blocking=True)
        dbuf = stage_l.to(DEV, non_blocking=True)
        c, o = part(dbuf, spans_l, "counts", torch.int32), part(dbuf, spans_l, "offsets", torch.int32)
        rle_kernels(rgb, c, o, torch.empty_like(c), part(dbuf, spans_l, "boxes", torch.int64), part(dbuf, spans_l, "im_id", torch.int32),
                    out_l, err)

    def host_string():
        rgb = h_rgb.to(DEV, non_blocking=True)
        dbuf = torch.empty(device_bytes, dtype=torch.uint8, device=DEV)
        dbuf[:stage_s.numel()].copy_(stage_s, non_blocking=True)
        c, o = part(dbuf, spans_s, "counts", torch.int32), part(dbuf, spans_s, "offsets", torch.int32)
        string_kernels(rgb, part(dbuf, spans_s, "bytes", torch.uint8), part(dbuf, spans_s, "byte_offsets", torch.int32), c, o,
                       torch.empty_like(c), part(dbuf, spans_s, "boxes", torch.int64), part(dbuf, spans_s, "im_id", torch.int32), out_s, err)

    t = measure({"list": host_list, "string": host_string}, args.reps, args.warmup)
    assert int(err.item()) == 0
    same = all(torch.equal(a, b) for a, b in zip(out_l, out_s))
    say()
    say(f"2. host to crops (copies + kernels), {args.reps} repetitions after {args.warmup} warm-ups, routes alternating")
    say(f"   list   : {stats(t['list'])}")
    say(f"   string : {stats(t['string'])}")
    say(f"   string / list = {np.median(t['string']) / np.median(t['list']):.3f}")
    say(f"   outputs of the two routes equal bit for bit: {same}")

    def scans(name, data, byte_offsets, counts, offsets):
        d_data, d_bo = torch.from_numpy(data).to(DEV), torch.from_numpy(byte_offsets).to(DEV)
        d_c, d_o = torch.from_numpy(counts).to(DEV), torch.from_numpy(offsets).to(DEV)
        d_x = torch.zeros_like(d_c)                    # the string scan's in/out slots
        cum_l, cum_s = torch.empty_like(d_c), torch.empty_like(d_c)
        no_bytes = torch.zeros_like(d_bo)
        t = measure({"list": lambda: list_scan(d_c, d_o, cum_l, H, W, err),
                     "string": lambda: string_scan(d_data, d_bo, d_o, d_x, cum_s, H, W, err),
                     "mixed": lambda: string_scan(d_data, no_bytes, d_o, d_c, cum_s, H, W, err)}, args.reps, args.warmup)
        string_scan(d_data, d_bo, d_o, d_x, cum_s, H, W, err)
        equal = torch.equal(cum_l, cum_s) and torch.equal(d_x, d_c) and int(err.item()) == 0
        say(f"   gpi_rle_scan, int32 lists            : {stats(t['list'])}")
        say(f"   gps_rle_string_scan, strings         : {stats(t['string'])}")
        say(f"   gps_rle_string_scan, the same lists  : {stats(t['mixed'])}")
        ratio = np.median(t["string"]) / np.median(t["list"])
        say(f"   string / list = {ratio:.3f}   expectation: within 2 x -> {'met' if ratio <= 2.0 else 'NOT met'}   counts and cum equal: {equal}")
        return equal

    say()
    say("3. scans alone (inputs resident), the workload above")
    same &= scans("workload", data, byte_offsets, counts, offsets)
    rng = np.random.RandomState(7)
    wc = ingest.mask_to_rle_counts(rng.rand(H, W) < 0.5)
    ws = rs.rle_string_from_counts(wc)
    w_packed = rs.pack_rle_any([dict(counts=ws, size=[H, W])], H, W)
    say()
    say(f"4. scans alone, one 50 % random mask: {len(wc)} runs in {len(ws)} string bytes against {4 * len(wc)} as int32; no expectation")
    same &= scans("noise", w_packed[0], w_packed[1], wc, w_packed[3])

    t0 = time.perf_counter()
    decoded = [ref.decode_counts(s) for s in strings]
    t1 = time.perf_counter()
    ingest.pack_rle([dict(counts=c, size=[H, W]) for c in decoded], H, W)
    t2 = time.perf_counter()
    vectorised = [rs.rle_counts_from_string(s) for s in strings]
    t3 = time.perf_counter()
    rs.pack_rle_any([dict(counts=s, size=[H, W]) for s in strings], H, W)
    t4 = time.perf_counter()
    assert all((a == b).all() for a, b in zip(decoded, vectorised))
    say()
    say("5. host cost of the same 64 strings (wall clock, one pass, one core)")
    say(f"   sequential Python decode {1e3 * (t1 - t0):8.1f} ms  + pack_rle {1e3 * (t2 - t1):6.1f} ms   (what a user without this route pays)")
    say(f"   vectorised numpy decode  {1e3 * (t3 - t2):8.1f} ms")
    say(f"   pack_rle_any             {1e3 * (t4 - t3):8.1f} ms   (the string route's whole host share)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
