"""Appearance-score measurement (needs one MI355X): the kernels of libgigapose_appear.so one by one, proposals.ProposalLabeller.label with
and without a PatchBank, and the same score written in torch ops on the same GPU.

Workload (seeded, generated here): --proposals 200 elliptic mask proposals on one 480 x 640 frame, a randomly initialised ViT-L/14
(C = 1024), a bank of --objects 40 x --templates 42 templates of random unit patch descriptors (quantised, split into limbs on the
device; made without the ViT: 1 680 forward passes say nothing about this stage) with random valid patches.  Stages, each timed
with HIP events, alternating inside every one of --reps repetitions after --warmup warm-ups:
  cls_only          Dinov2ViT.cls_descriptors: the forward in chunks of 64 + gpa_descriptors (what the labeller runs without a PatchBank)
  cls_and_patches   Dinov2ViT.cls_and_patch_descriptors: the same forwards + gpa_descriptors + gpp_patch_descriptors + gpp_patch_valid
  patch_tokens      gpp_patch_descriptors alone, on the workspace the last forward left
  patch_valid       gpp_patch_valid alone, on the crops' masks
  appearance        gpp_appearance: one (crop, best template) pair per proposal
  torch_appearance  the same score in torch ops: gather the bank rows, f32 bmm, masked max, mean (no integers: ties and the last bits differ)
and ProposalLabeller.label as a whole by the wall clock, with and without the PatchBank.  Every step runs under a time limit of its
own (--limit seconds, SIGALRM): a step that hangs ends the run.

No time is required of this stage: there is no earlier code to compare with.  The run fails if sums, counts or flags differ from the
numpy restatement.  Writes --out (default profiles/appearance_scores.txt)."""
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
from gigapose_amd import appearance, ingest, proposals  # noqa: E402
from gigapose_amd.vit import VARIANTS, Dinov2ViT  # noqa: E402
from gigapose_testing import appear_ref as ref  # noqa: E402
from gigapose_testing import label_cases  # noqa: E402
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


def limbs_on_device(q):
    """q int32 (..) within 2^20 on the device -> int8 (3, ..): the header's balanced base-128 digits."""
    a0 = ((q + 64) & 127) - 64
    q1 = (q - a0) >> 7
    a1 = ((q1 + 64) & 127) - 64
    return torch.stack([a0, a1, (q1 - a1) >> 7]).to(torch.int8)


def random_patch_bank(O, T, C, seed, vit):
    """A PatchBank of random unit patch descriptors, one object at a time on the device; ~55 % of the patches valid, patch 0 always."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    bank = appearance.PatchBank(vit)
    for o in range(O):
        v = torch.randn(T, 256, C, device=DEV, generator=gen, dtype=torch.float64)
        q = torch.round(v / v.norm(dim=2, keepdim=True) * float(1 << 20)).to(torch.int32)
        valid = (torch.rand(T, 256, device=DEV, generator=gen) < 0.55).to(torch.uint8)
        valid[:, 0] = 1
        bank.labels.append(o + 1)
        bank._a.append(limbs_on_device(q))
        bank._valid.append(valid)
    return bank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "appearance_scores.txt"))
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
        bank_q = label_cases.quantise(label_cases.unit_vectors(rs, O * T, dim)).reshape(O, T, dim)
        bank = proposals.DescriptorBank.from_arrays(bank_q, np.arange(1, O + 1), device=DEV, vit=vit)
        patches = random_patch_bank(O, T, dim, 12, vit)
        frame = torch.from_numpy(rs.randint(0, 256, size=(1, 3, H, W)).astype(np.uint8))
        props = elliptic_proposals(rs, P)
        plain = proposals.ProposalLabeller(vit, bank, top_k=args.top_k, min_score=-1.0)
        labeller = proposals.ProposalLabeller(vit, bank, top_k=args.top_k, min_score=-1.0, appearance=patches)
        d = labeller.describe(frame, [props])                          # also the first warm-up of every kernel
        torch.cuda.synchronize()
    crops, masks, qa, q_valid, pair_t = d["crops"], d["tar_mask"], d["a"], d["pvalid"], d["pair_t"]
    ta, t_valid = patches.a, patches.valid
    qi = torch.arange(P, dtype=torch.int32, device=DEV)
    gamma, beta = vit.norm.weight.detach().float().contiguous(), vit.norm.bias.detach().float().contiguous()
    n_last = P - (P - 1) // 64 * 64                                    # the crops of the last chunk are what the workspace holds
    mpad = (n_last * 257 + 255) // 256 * 256
    scale = 2.0 ** -20
    qf = (qa[0].float() + 128.0 * qa[1].float() + 16384.0 * qa[2].float()) * scale          # (P, 256, C) f32
    live_q = q_valid != 0

    def torch_appearance():
        rows = pair_t.long()
        tf = (ta[0, rows].float() + 128.0 * ta[1, rows].float() + 16384.0 * ta[2, rows].float()) * scale
        sim = torch.bmm(qf, tf.transpose(1, 2)).masked_fill((t_valid[rows] == 0)[:, None, :], float("-inf"))
        top, at = sim.max(dim=2)
        return (top * live_q).sum(dim=1) / live_q.sum(dim=1).clamp(min=1), at

    stages = {
        "cls_only": lambda: vit.cls_descriptors(crops),
        "cls_and_patches": lambda: vit.cls_and_patch_descriptors(crops, masks),
        "patch_tokens": lambda: appearance.patch_descriptors(vit._ws, 257, 1, mpad, gamma, beta, vit.norm.eps, n_last, dim, offset=1),
        "patch_valid": lambda: appearance.patch_valid(masks),
        "appearance": lambda: appearance.appearance(qa, q_valid, ta, t_valid, qi, pair_t),
        "torch_appearance": torch_appearance,
    }
    with limit("the timed stages", args.limit * (args.reps + args.warmup)):
        times = pt.measure(stages, args.reps, args.warmup)
    wall = {"without": [], "with": []}
    with limit("ProposalLabeller.label", args.limit * 4):
        for _ in range(1 + 3):
            for name, lab in (("without", plain), ("with", labeller)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lab.label(frame, [props])
                wall[name].append((time.perf_counter() - t0) * 1e3)
    # the restatement on the device's own limbs: sums, counts, flags, argmaxes
    with limit("the restatement", args.limit * 2):
        got = appearance.appearance(qa, q_valid, ta, t_valid, qi, pair_t, want=("arg",))
        rows = pair_t.long()
        want = ref.appearance(qa.cpu().numpy(), q_valid.cpu().numpy(), ta[:, rows].cpu().numpy(), t_valid[rows].cpu().numpy(), np.arange(P), np.arange(P))
        same = all(got[k].cpu().numpy().tobytes() == want[k].tobytes() for k in ("sum", "n", "status", "arg"))
        t_score, t_arg = torch_appearance()
        score = ref.float_appearance(want["sum"], want["n"])
        dev_max = float(np.abs(t_score.cpu().numpy().astype(np.float64) - score).max())
        differ = int(((t_arg.cpu().numpy() != want["arg"]) & (q_valid.cpu().numpy() != 0)).sum())
        n_valid = int((q_valid != 0).sum())
    macs = P * 256 * 256 * dim
    lines = [f"device: {torch.cuda.get_device_name(0)}; commit {pt.commit()}",
             f"{args.reps} repetitions after {args.warmup} warm-ups, HIP events around each stage, the stages alternating inside every repetition; times in us",
             f"workload: {P} proposals on one {H} x {W} frame, {args.variant} (C = {dim}, random weights), patch bank {O} objects x {T} templates "
             f"({ta.numel() / 1e6:.0f} MB of limbs), one (crop, best template) pair per proposal, {n_valid} valid query patches", ""]
    what = {"cls_only": f"the ViT forward in {-(-P // 64)} chunks + gpa_descriptors",
            "cls_and_patches": "the same forwards + gpa_descriptors + gpp_patch_descriptors + gpp_patch_valid",
            "patch_tokens": f"gpp_patch_descriptors alone, {n_last} crops = {n_last * 256} tokens",
            "patch_valid": f"gpp_patch_valid alone, {P} crop masks",
            "appearance": f"gpp_appearance: {P} pairs x 256 x 256 x {dim} = {macs:.2e} exact products, 9 int8 MFMA limb products each",
            "torch_appearance": "gather of the bank rows + f32 bmm + masked max + mean in torch ops"}
    lines += [pt.line(k, times[k], what[k], width=16) for k in stages]
    med = float(np.median(times["appearance"]))
    lines += ["", f"gpp_appearance: {9 * 2 * macs / med / 1e6:.1f} int8 TOP/s over the nine limb products ({macs / med / 1e6:.1f} T exact 21-bit multiply-adds per second)",
              f"ProposalLabeller.label as a whole (host packing, uploads, kernels, read-back; wall clock, 3 runs after one): without a PatchBank median "
              f"{np.median(wall['without'][1:]):.1f} ms (min {min(wall['without'][1:]):.1f}), with one median {np.median(wall['with'][1:]):.1f} ms "
              f"(min {min(wall['with'][1:]):.1f}); {labeller.report}",
              f"torch's f32 score differs from the integer score by at most {dev_max:.2e}; its argmax differs for {differ} of {n_valid} valid query patches",
              f"sums, counts, flags and argmaxes equal the restatement: {same}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    if not same:
        raise SystemExit("the device results differ from the restatement")


if __name__ == "__main__":
    main()
