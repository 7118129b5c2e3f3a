"""Detection-scoring measurement (needs one MI355X): the kernels of libgigapose_coco.so one by one and detections.DetectionScorer.score as
a whole, beside two baselines that are references and never the code under test.

Workload (seeded, generated here, the shape of profiles/verify_hypotheses.txt): --images 100 frames of 480 x 640, each with
--per-image 15 elliptic ground truths of 5 categories and as many detections (the ground truths moved by a few pixels): 1 500
detections, 1 500 ground truths, masks of about 200 runs, every detection paired with the ground truths of its image and category.
Stages, each timed with HIP events, alternating inside every one of --reps repetitions after --warmup warm-ups:
  fg_scan      gpc_fg_scan over the detections' and the ground truths' lists
  mask_inter   gpc_mask_inter over all pairs
  match        gpc_match over all (image, category) groups at 10 thresholds
  torch_dense  the same intersections by torch on the device from DENSE bool masks that are already there (decoding them is not
               counted): (a & b).sum per pair, gathered in chunks
and, by the wall clock: the numpy restatement (coco_ref: fg_scan + mask_inter + match) on one host thread, and a whole
DetectionScorer.score (host grouping, packing, uploads, kernels, read-back, the AP arithmetic).  Every step runs under a time limit
of its own (--limit seconds, SIGALRM): a step that hangs ends the run.

No time is required of this stage: there is no earlier code to compare with.  The run fails if the intersections differ from the
dense ones or the matches from the restatement.  Writes --out (default profiles/detection_scores.txt)."""
import argparse
import contextlib
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import detections  # noqa: E402
from gigapose_testing import coco_cases as cases  # noqa: E402
from gigapose_testing import coco_ref as ref  # noqa: E402
from gigapose_testing import probe_timing as pt  # noqa: E402

DEV = "cuda"
H, W = 480, 640


@contextlib.contextmanager
def limit(name, seconds):
    def expired(*_):
        raise SystemExit(f"step `{name}` did not finish within {seconds} s")

    signal.signal(signal.SIGALRM, expired)
    signal.alarm(int(seconds))
    try:
        yield
    finally:
        signal.alarm(0)


def ellipse_runs(cx, cy, rx, ry):
    """The run list of a filled ellipse, column by column, without the dense mask."""
    xs = np.arange(max(0, int(np.ceil(cx - rx))), min(W - 1, int(np.floor(cx + rx))) + 1)
    half = ry * np.sqrt(np.maximum(0.0, 1.0 - ((xs - cx) / rx) ** 2))
    ya, yb = np.maximum(0, np.ceil(cy - half).astype(np.int64)), np.minimum(H - 1, np.floor(cy + half).astype(np.int64))
    ok = yb >= ya
    a, b = (xs * H + ya)[ok], (xs * H + yb + 1)[ok]                    # the columns' pixel ranges [a, b): ascending, apart
    edges = np.concatenate(([0], np.stack([a, b], axis=1).reshape(-1), [H * W]))
    return np.diff(edges).tolist()


def workload(rs, n_img, per_image):
    gts, dets, objects = {}, {}, {}
    for im in range(n_img):
        rows, listed = [], []
        for n in range(per_image):
            e = (rs.uniform(70, W - 70), rs.uniform(70, H - 70), rs.uniform(35, 60), rs.uniform(35, 60))
            counts = ellipse_runs(*e)
            box = [int(e[0] - e[2]), int(e[1] - e[3]), int(2 * e[2]), int(2 * e[3])]
            rows.append(dict(obj_id=1 + n % 5, visib_fract=float(rs.uniform(0.0, 1.0)), bbox_visib=box, mask_visib=dict(size=[H, W], counts=counts)))
            moved = ellipse_runs(e[0] + rs.uniform(-12, 12), e[1] + rs.uniform(-12, 12), e[2], e[3])
            listed.append(dict(category_id=1 + n % 5, score=float(rs.uniform(0.0, 1.0)), bbox=box, segmentation=dict(size=[H, W], counts=moved)))
        gts[(1, im)], dets[(1, im)] = rows, listed
    return gts, dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detection_scores.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--per-image", type=int, default=15)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    args = ap.parse_args()
    rs = np.random.RandomState(17)
    with limit("set-up", 2 * args.limit):
        gts, dets = workload(rs, args.images, args.per_image)
        keys = sorted(gts)
        det_lists = [np.asarray(d["segmentation"]["counts"], np.int32) for k in keys for d in dets[k]]
        gt_lists = [np.asarray(r["mask_visib"]["counts"], np.int32) for k in keys for r in gts[k]]
        (dcum, doff), (gcum, goff) = cases.pack_cum(det_lists), cases.pack_cum(gt_lists)
        # groups in the scorer's order: image, category; detections best first, ignored ground truths last
        groups, pair_a, pair_b = [], [], []
        for i, k in enumerate(keys):
            for c in range(1, 6):
                dt = sorted((n for n, d in enumerate(dets[k]) if d["category_id"] == c), key=lambda n: -dets[k][n]["score"])
                gt = sorted((n for n, r in enumerate(gts[k]) if r["obj_id"] == c), key=lambda n: gts[k][n]["visib_fract"] < 0.1)
                groups.append(([i * args.per_image + n for n in dt], [i * args.per_image + n for n in gt], [gts[k][n]["visib_fract"] < 0.1 for n in gt]))
        det_sel = np.asarray([n for g in groups for n in g[0]], np.int64)
        gt_sel = np.asarray([n for g in groups for n in g[1]], np.int64)
        for dt, gt, _ in groups:
            pair_a += [d for d in dt for _ in gt]
            pair_b += [g for _ in dt for g in gt]
        pair_a, pair_b = np.asarray(pair_a, np.int32), np.asarray(pair_b, np.int32)
        D, G = np.asarray([len(g[0]) for g in groups]), np.asarray([len(g[1]) for g in groups])
        det_off, gt_off = (np.concatenate(([0], np.cumsum(v))).astype(np.int32) for v in (D, G))
        pair_off = np.concatenate(([0], np.cumsum(D * G)))[:-1].astype(np.int32)
        ignore = np.asarray([f for g in groups for f in g[2]], np.uint8)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        dl, gl = (t(dcum), t(doff)), (t(gcum), t(goff))
        pa, pb = t(pair_a), t(pair_b)
        dense_d = torch.stack([t(cases.decode(c, H * W)) for c in det_lists])
        dense_g = torch.stack([t(cases.decode(c, H * W)) for c in gt_lists])
        dfg, gfg = detections.foreground(dl, H * W), detections.foreground(gl, H * W)
        inter, status = detections.mask_intersections(dfg, gfg, pa, pb)
        area_det, area_gt = dfg.area[t(det_sel)].contiguous(), gfg.area[t(gt_sel)].contiguous()
        margs = (t(det_off), t(gt_off), t(pair_off), inter, area_det, area_gt, t(ignore), cases.THRESHOLDS, cases.THR_DEN)
        got = detections.match(*margs)
        torch.cuda.synchronize()

    def torch_dense(chunk=1500):
        return torch.cat([(dense_d[pa[a:a + chunk].long()] & dense_g[pb[a:a + chunk].long()]).sum(dim=1) for a in range(0, len(pair_a), chunk)])

    stages = {
        "fg_scan": lambda: (detections.foreground(dl, H * W), detections.foreground(gl, H * W)),
        "mask_inter": lambda: detections.mask_intersections(dfg, gfg, pa, pb),
        "match": lambda: detections.match(*margs),
        "torch_dense": torch_dense,
    }
    with limit("the timed stages", args.limit * (args.reps + args.warmup)):
        times = pt.measure(stages, args.reps, args.warmup)
    with limit("the restatement", args.limit * 4):
        t0 = time.perf_counter()
        rd, rg = ref.fg_scan(dcum, doff, H * W), ref.fg_scan(gcum, goff, H * W)
        t1 = time.perf_counter()
        r_inter, _ = ref.mask_inter((dcum, doff, rd[0]), (gcum, goff, rg[0]), H * W, pair_a, pair_b)
        t2 = time.perf_counter()
        want = ref.match(det_off, gt_off, pair_off, r_inter, rd[1][det_sel], rg[1][gt_sel], ignore, list(cases.THRESHOLDS), cases.THR_DEN)
        t3 = time.perf_counter()
        same = inter.cpu().numpy().tobytes() == r_inter.tobytes() and torch.equal(inter, torch_dense()) and not int(status.max())
        same = same and all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(got, want))
    wall = []
    with limit("DetectionScorer.score", args.limit * 4):
        scorer = detections.DetectionScorer(gts)
        for _ in range(1 + 3):
            torch.cuda.synchronize()
            t0s = time.perf_counter()
            out = scorer.score(dets)
            wall.append((time.perf_counter() - t0s) * 1e3)
    runs = (len(dcum) + len(gcum)) / (len(det_lists) + len(gt_lists))
    lines = [f"device: {torch.cuda.get_device_name(0)}; commit {pt.commit()}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each stage, the stages alternating inside every repetition; times in us",
             f"workload: {args.images} frames of {H} x {W}, {len(det_lists)} detections x the ground truths of their image and category ({len(gt_lists)} in all): "
             f"{len(pair_a)} pairs in {len(groups)} groups, {runs:.0f} runs per mask on average", ""]
    what = {"fg_scan": f"gpc_fg_scan, {len(det_lists)} + {len(gt_lists)} masks (two calls)", "mask_inter": f"gpc_mask_inter, {len(pair_a)} pairs",
            "match": f"gpc_match, {len(groups)} groups x 10 thresholds", "torch_dense": "(a & b).sum(1) of dense bool masks already on the device, torch ops"}
    lines += [pt.line(k, times[k], what[k]) for k in stages]
    med = {k: float(np.median(times[k])) for k in stages}
    lines += ["", f"the numpy restatement on one host thread (wall clock, one run): fg_scan {(t1 - t0) * 1e3:.1f} ms, mask_inter {(t2 - t1) * 1e3:.1f} ms, "
              f"match {(t3 - t2) * 1e3:.1f} ms",
              f"DetectionScorer.score as a whole (host grouping, packing, uploads, kernels, read-back, AP; wall clock, 3 runs after one): median "
              f"{np.median(wall[1:]):.1f} ms (min {min(wall[1:]):.1f}); AP {out['AP']:.4f} AP50 {out['AP50']:.4f} AP75 {out['AP75']:.4f} AR {out['AR']:.4f}",
              f"run-length route (fg_scan + mask_inter) against the dense torch route: {med['fg_scan'] + med['mask_inter']:.1f} us against {med['torch_dense']:.1f} us "
              f"({'faster' if med['fg_scan'] + med['mask_inter'] < med['torch_dense'] else 'NOT faster'})",
              f"intersections equal the dense ones and the restatement's, matches equal the restatement's: {same}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not same:
        raise SystemExit("the device results differ from the references")


if __name__ == "__main__":
    main()
