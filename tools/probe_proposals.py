"""Proposal-labelling measurement (needs one MI355X): the stages of proposals.ProposalLabeller.label one by one, and the scoring
written in torch ops on the same GPU beside gpa_scores.

Workload (seeded, generated here): --proposals 200 elliptic mask proposals on one 480 x 640 frame, a bank of --objects 40 x
--templates 42 random unit descriptors (quantised; made without the ViT: 1 680 forward passes say nothing about this stage), a
randomly initialised ViT-L/14 (C = 1024) for the descriptors.  Stages, each timed with HIP events, alternating inside every one of
--reps repetitions after --warmup warm-ups:
  boxes        gpi_rle_scan + gpa_run_boxes over the proposals' run lists
  crops        ingest.RleDetectionPreprocessor (scan + crop) at the boxes found
  descriptors  Dinov2ViT.cls_descriptors: the forward in chunks of 64 + gpa_descriptors
  layer_norm   gpa_descriptors alone, on the workspace the last forward left
  scores       gpa_scores (dots + selection)
  torch_scores the same scoring in torch ops: f32 matmul, topk, mean, max (no integers: ties and the last bits differ)
  nms          gpa_nms_matrix + gpa_nms_keep over all proposals in score order
and ProposalLabeller.label as a whole by the wall clock (host packing, uploads, kernels, read-back).  Every step runs under a time
limit of its own (--limit seconds, SIGALRM): a step that hangs ends the run.

No time is required of this stage: there is no earlier code to compare with.  The run fails if labels, scores or kept boxes differ
from the numpy restatement.  Writes --out (default profiles/proposal_labels.txt)."""
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
from gigapose_amd import ingest, proposals  # noqa: E402
from gigapose_amd.vit import VARIANTS, Dinov2ViT  # noqa: E402
from gigapose_testing import label_cases as cases  # noqa: E402
from gigapose_testing import label_ref as ref  # noqa: E402
from gigapose_testing import probe_timing as pt  # noqa: E402
from gigapose_testing import synthetic as syn  # noqa: E402

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


def elliptic_proposals(rs, n):
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        cx, cy, rx, ry = rs.uniform(40, W - 40), rs.uniform(40, H - 40), rs.uniform(10, 90), rs.uniform(10, 90)
        m = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
        out.append(dict(segmentation=dict(counts=ingest.mask_to_rle_counts(m).tolist(), size=[H, W])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_labels.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--proposals", type=int, default=200)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--templates", type=int, default=42)
    ap.add_argument("--variant", default="dinov2_vitl14")
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    args = ap.parse_args()
    rs = np.random.RandomState(11)
    P, O, T = args.proposals, args.objects, args.templates
    dim, depth, heads = VARIANTS[args.variant]
    with limit("set-up", 4 * args.limit):
        vit = syn.fill_state_dict(Dinov2ViT(dim, depth, heads), 5).eval().to(DEV)
        bank_q = cases.quantise(cases.unit_vectors(rs, O * T, dim)).reshape(O, T, dim)
        bank = proposals.DescriptorBank.from_arrays(bank_q, np.arange(1, O + 1), device=DEV, vit=vit)
        frame = torch.from_numpy(rs.randint(0, 256, size=(1, 3, H, W)).astype(np.uint8))
        props = elliptic_proposals(rs, P)
        labeller = proposals.ProposalLabeller(vit, bank, top_k=args.top_k, min_score=-1.0)
        d = labeller.describe(frame, [props])                          # also the first warm-up of every kernel
        torch.cuda.synchronize()
    counts, offsets = ingest.pack_rle([p["segmentation"] for p in props], H, W)
    counts_d, offsets_d = torch.from_numpy(counts).to(DEV), torch.from_numpy(offsets).to(DEV)
    frame_d, crops, q = frame.to(DEV), d["crops"], d["q"]
    boxes, im_id = d["box"], np.zeros(P, np.int32)
    gamma, beta = vit.norm.weight.detach().float().contiguous(), vit.norm.bias.detach().float().contiguous()
    n_last = P - (P - 1) // 64 * 64                                    # the crops of the last chunk are what the workspace holds
    mpad = (n_last * 257 + 255) // 256 * 256
    order = torch.sort(d["score_dev"], descending=True, stable=True).indices
    box32 = torch.from_numpy(boxes.astype(np.int32)).to(DEV)[order].contiguous()
    label32 = torch.from_numpy(d["label"]).to(DEV)[order].contiguous()
    qf = q.float() / 2.0 ** 20
    bf = bank.q.float().reshape(O * T, dim) / 2.0 ** 20
    kk = min(args.top_k, T)

    def torch_scores():
        obj = (qf @ bf.t()).reshape(P, O, T).topk(kk, dim=2).values.mean(dim=2)
        return obj.max(dim=1)

    stages = {
        "boxes": lambda: proposals.mask_boxes(counts_d, offsets_d, H, W),
        "crops": lambda: labeller.preprocess(frame_d, counts_d, offsets_d, boxes, im_id),
        "descriptors": lambda: vit.cls_descriptors(crops),
        "layer_norm": lambda: proposals.descriptors(vit._ws, 257, mpad, gamma, beta, vit.norm.eps, n_last, dim),
        "scores": lambda: proposals.scores(q, bank.q, args.top_k),
        "torch_scores": torch_scores,
        "nms": lambda: proposals.nms(box32, label32, 1, 4),
    }
    with limit("the timed stages", args.limit * (args.reps + args.warmup)):
        times = pt.measure(stages, args.reps, args.warmup)
    wall = []
    with limit("ProposalLabeller.label", args.limit * 4):
        for _ in range(1 + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dets = labeller.label(frame, [props])
            wall.append((time.perf_counter() - t0) * 1e3)
    # the restatement on the device's own descriptors: labels, scores, the kept set and its order
    with limit("the restatement", args.limit * 2):
        sc = ref.scores(q.cpu().numpy(), bank_q, args.top_k)
        got = proposals.scores(q, bank.q, args.top_k)
        same = all(got[k].cpu().numpy().tobytes() == sc[k].tobytes() for k in ("label", "score", "best_template"))
        want, report = ref.label_proposals(im_id, sc, d["dstatus"], d["mstatus"], boxes, sc["kk"], -1.0, (1, 4), False, None, 1)
        same = same and [x["proposal"] for x in dets[0]] == want[0] and report == labeller.report
        ts_val, ts_idx = torch_scores()
        agree = int((ts_idx.cpu().numpy() == sc["label"]).sum())
        dev_max = float(np.abs(ts_val.cpu().numpy().astype(np.float64) - ref.float_score(sc["score"], sc["kk"])).max())
    lines = [f"device: {torch.cuda.get_device_name(0)}; commit {pt.commit()}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each stage, the stages alternating inside every repetition; times in us",
             f"workload: {P} proposals on one {H} x {W} frame ({len(counts)} runs), bank {O} objects x {T} templates, {args.variant} (C = {dim}, random weights), "
             f"top_k = {args.top_k}", ""]
    what = {"boxes": "gpi_rle_scan + gpa_run_boxes", "crops": "gpi_rle_scan + gpi_preprocess_detections_rle (one host sync)",
            "descriptors": f"the ViT forward in {-(-P // 64)} chunks + gpa_descriptors", "layer_norm": f"gpa_descriptors alone, {n_last} crops",
            "scores": f"gpa_scores: {P} x {O * T} x {dim} exact int64 dots + top-{kk} + argmax",
            "torch_scores": "f32 matmul + topk + mean + max in torch ops", "nms": f"gpa_nms_matrix + gpa_nms_keep, {P} boxes"}
    lines += [pt.line(k, times[k], what[k]) for k in stages]
    lines += ["", f"ProposalLabeller.label as a whole (host packing, uploads, kernels, read-back; wall clock, 3 runs after one): median {np.median(wall[1:]):.1f} ms "
              f"(min {min(wall[1:]):.1f}); {labeller.report}",
              f"torch's f32 scoring picks the integer scoring's label for {agree} of {P} proposals; its scores differ by at most {dev_max:.2e}",
              f"labels, scores, best templates, the kept proposals and their order equal the restatement: {same}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not same:
        raise SystemExit("the device results differ from the restatement")


if __name__ == "__main__":
    main()
