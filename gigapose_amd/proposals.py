"""Mask proposals in, labelled detections out: what stands between a class-agnostic segmenter (SAM, FastSAM, anything that gives
masks) and ingest.FrameIngest, whose detections carry a `category_id` and a `score` (libgigapose_label.so, C-ABI:
include/gigapose_label.h).

It is the matching stage of CNOS, for objects onboarded here: a proposal is cropped as a detection is (rgb x mask, 224 x 224, CLIP
normalisation: ingest.RleDetectionPreprocessor), described by the class token of a DINOv2 ViT after the final LayerNorm,
L2-normalised (Dinov2ViT.cls_descriptors), compared by cosine similarity with the descriptors of every template of every object; an
object's score is the mean of its top k templates, the label the best object; low scores are dropped and a greedy box NMS removes
duplicates.  Every decision is taken on integers (descriptors are quantised to 2^-20, the similarities are exact int64 sums), so
the labels do not depend on launch geometry; gigapose_testing/label_ref.py restates the arithmetic and agrees bit for bit.

  descriptors(x, ...)                  class tokens (any strides) -> (q int32 (B, C), status)            gpa_descriptors
  scores(q, bank_q, k)                 -> label, score, best_template (+ dot, obj)                       gpa_scores
  mask_boxes(counts, offsets, H, W)    run-length masks -> tight boxes, areas, status                    gpi_rle_scan + gpa_run_boxes
  nms(box, label, num, den, per_label) boxes in suppression order -> keep                                gpa_nms_matrix + gpa_nms_keep
  DescriptorBank                       the descriptors of the onboarded objects' templates, (O, T, C)
  ProposalLabeller                     frames + proposals -> per image the list of CNOS dicts FrameIngest takes
The appearance score of CNOS's successors (patch-level similarity with the best template: appearance.py, libgigapose_appear.so) is
averaged into the score when ProposalLabeller is given a PatchBank.  Out of scope: the segmenter, CNOS's visibility / geometric score,
objects with different template counts.  (A mask-IoU NMS is detections.mask_nms; ProposalLabeller(nms_on="mask") routes through it.)  There is no CPU fallback: the kernels need the GPU, a missing library is an error.
"""
import numpy as np
import torch

from . import _lib
from .ingest import RleDetectionPreprocessor, pack_rle, xywh_to_xyxy_long
from .ingest import _call as _ingest_call

Q_BITS = 20
NON_FINITE, ZERO_NORM = 1, 2          # status bits of descriptors (GPA_NON_FINITE, GPA_ZERO_NORM)
EMPTY_MASK, BAD_MASK = 1, 2           # status bits of mask_boxes (GPA_EMPTY_MASK, GPA_BAD_MASK)
MAX_C, MAX_K, MAX_BANK, MAX_NMS = 2048, 64, 1 << 20, 8192
MAX_MASKS_PER_CALL = 65535            # the grid's first dimension is not the limit: gpi_rle_scan's D is
DOT_BYTES_PER_CALL = 1 << 28          # scores() chunks the proposals so that dot (P, O, T) int64 stays below this
_label = _lib.SideLibrary("libgigapose_label.so", "gpa")
LABEL_LIB_PATH, lib, _call = _label.path, _label.lib, _label.call


# ------------------------------------------------------------------------------------------------ the kernels, one wrapper each
@torch.no_grad()
def descriptors(x, crop_stride, channel_stride, gamma, beta, eps, B, C):
    """x: an f32 tensor on the device whose storage holds value c of crop b's class token at element b * crop_stride + c *
    channel_stride from x's first element -> (q int32 (B, C), status int32 (B)).  gamma, beta: the LayerNorm's f32 (C)."""
    who = "descriptors"
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32):
        raise ValueError(f"{who}: x must be a float32 tensor")
    B, C, crop_stride, channel_stride = int(B), int(C), int(crop_stride), int(channel_stride)
    if not (C >= 64 and C <= MAX_C and C % 64 == 0):
        raise ValueError(f"{who}: C = {C} channels (a multiple of 64, 64 to {MAX_C})")
    if B < 0 or crop_stride <= 0 or channel_stride <= 0:
        raise ValueError(f"{who}: bad sizes B = {B}, strides {crop_stride}, {channel_stride}")
    if B and (B - 1) * crop_stride + (C - 1) * channel_stride >= x.numel():
        raise ValueError(f"{who}: the strides leave x ({x.numel()} elements)")
    gamma, beta = _lib.arg(gamma, torch.float32, (C,), who, "gamma"), _lib.arg(beta, torch.float32, (C,), who, "beta")
    _lib.on_gpu(who, x=x, gamma=gamma, beta=beta)
    if not x.is_contiguous():
        raise ValueError(f"{who}: x is not contiguous (the strides are passed, not taken from the tensor)")
    q = torch.empty(B, C, dtype=torch.int32, device=x.device)
    status = torch.empty(B, dtype=torch.int32, device=x.device)
    _call("gpa_descriptors", x, crop_stride, channel_stride, gamma, beta, eps, B, C, q, status, _lib.stream_ptr())
    return q, status


@torch.no_grad()
def scores(q, bank_q, k, want=()):
    """q (P, C), bank_q (O, T, C) int32 on the device -> dict(label int32 (P), score int64 (P), best_template int32 (P), kk):
    include/gigapose_label.h's gpa_scores.  want: "obj" and / or "dot" add those tensors."""
    who = "scores"
    if not (isinstance(bank_q, torch.Tensor) and bank_q.dim() == 3):
        raise ValueError(f"{who}: bank_q must be an (O, T, C) tensor")
    O, T, C = bank_q.shape
    q, bank_q = _lib.arg(q, torch.int32, (None, C), who, "q"), _lib.arg(bank_q, torch.int32, (O, T, C), who, "bank_q")
    k = int(k)
    if not (O >= 1 and T >= 1 and O * T <= MAX_BANK and 1 <= C <= MAX_C and 1 <= k <= MAX_K):
        raise ValueError(f"{who}: bad sizes O = {O}, T = {T}, C = {C}, k = {k} (O, T >= 1, O*T <= 2^20, C <= {MAX_C}, 1 <= k <= {MAX_K})")
    _lib.on_gpu(who, q=q, bank_q=bank_q)
    P, dev = q.shape[0], q.device
    out = dict(label=torch.empty(P, dtype=torch.int32, device=dev), score=torch.empty(P, dtype=torch.int64, device=dev),
               best_template=torch.empty(P, dtype=torch.int32, device=dev), kk=min(k, T))
    obj = torch.empty(P, O, dtype=torch.int64, device=dev) if "obj" in want else None
    step = max(1, DOT_BYTES_PER_CALL // (8 * O * T))
    dot = torch.empty(P if "dot" in want else min(P, step), O, T, dtype=torch.int64, device=dev)
    for a in range(0, P, step):
        b = min(P, a + step)
        _call("gpa_scores", q[a:b], bank_q, b - a, O, T, C, k, dot[a:b] if "dot" in want else dot, None if obj is None else obj[a:b], out["label"][a:b],
              out["score"][a:b], out["best_template"][a:b], _lib.stream_ptr())
    if obj is not None:
        out["obj"] = obj
    if "dot" in want:
        out["dot"] = dot
    return out


def float_scores(score, kk):
    """The int64 sums as float64 mean cosines: score / (kk * 2^40), one correctly rounded division."""
    return score.to(torch.float64) / float(kk * (1 << (2 * Q_BITS)))


@torch.no_grad()
def run_boxes(cum, offsets, H, W):
    """cum int32[total], offsets int32[D+1] on the device (gpi_rle_scan's) -> (box int32 (D,4) xyxy with exclusive ends, area int64
    (D), status int32 (D))."""
    who = "run_boxes"
    cum, offsets = _lib.arg(cum, torch.int32, (None,), who, "cum"), _lib.arg(offsets, torch.int32, (None,), who, "offsets")
    H, W = int(H), int(W)
    if offsets.numel() < 1 or not (H > 0 and W > 0 and H * W < 2 ** 31):
        raise ValueError(f"{who}: bad sizes (offsets has D + 1 entries, 0 < H*W < 2^31)")
    _lib.on_gpu(who, cum=cum, offsets=offsets)
    D, dev = offsets.numel() - 1, cum.device
    box = torch.empty(D, 4, dtype=torch.int32, device=dev)
    area = torch.empty(D, dtype=torch.int64, device=dev)
    status = torch.empty(D, dtype=torch.int32, device=dev)
    for _, a, b in _lib.chunked(D, MAX_MASKS_PER_CALL):
        _call("gpa_run_boxes", cum, offsets[a:b + 1], cum.numel(), b - a, H, W, box[a:b], area[a:b], status[a:b], _lib.stream_ptr())
    return box, area, status


@torch.no_grad()
def mask_boxes(counts, offsets, H, W, device="cuda"):
    """Uncompressed run-length masks (ingest.pack_rle's counts int32[total], offsets int32[D+1]; numpy or tensors) -> (box, area,
    status) on the device, through gpi_rle_scan + gpa_run_boxes.  A bad list (a negative run, a total other than H*W) raises a
    ValueError that names the mask; an empty mask is no error: status EMPTY_MASK, box 0, 0, 0, 0."""
    return mask_boxes_and_lists(counts, offsets, H, W, device)[0]


@torch.no_grad()
def scan_lists(who, counts, offsets, H, W, device="cuda"):
    """counts, offsets as mask_boxes takes them -> (cum, offsets) on the device (gpi_rle_scan, chunked at 65535 masks) and `check`,
    which raises the ValueError of a bad list when called (a host synchronisation)."""
    (counts, ct), (offsets, ot) = _lib.checked(counts, torch.int32, (None,), who, "counts"), _lib.checked(offsets, torch.int32, (None,), who, "offsets")
    dev = counts.device if counts.is_cuda else device
    counts, offsets = _lib.upload(who, dev, (counts, ct), (offsets, ot))
    D = offsets.numel() - 1
    if D < 0:
        raise ValueError(f"{who}: offsets has D + 1 entries")
    err = torch.zeros(max(1, -(-D // MAX_MASKS_PER_CALL)), dtype=torch.int32, device=counts.device)
    cum = torch.empty_like(counts)
    for c, a, b in _lib.chunked(D, MAX_MASKS_PER_CALL):
        _ingest_call("gpi_rle_scan", counts, offsets[a:b + 1], counts.numel(), b - a, H, W, cum, err[c:c + 1], _lib.stream_ptr())

    def check():
        bad = _lib.first_bad(err.tolist(), MAX_MASKS_PER_CALL)
        if bad is not None:
            raise ValueError(f"{who}: mask {bad} has a bad run-length list (no run, a negative run or a total other than H*W = {H * W})")

    return cum, offsets, check


@torch.no_grad()
def mask_boxes_and_lists(counts, offsets, H, W, device="cuda"):
    """mask_boxes, and the scanned lists it was taken from: -> ((box, area, status), (cum, offsets))."""
    cum, offsets, check = scan_lists("mask_boxes", counts, offsets, H, W, device)
    out = run_boxes(cum, offsets, H, W)
    check()
    return out, (cum, offsets)


def _threshold(nms_iou):
    num, den = (int(v) for v in nms_iou)
    if not (1 <= den <= 65536 and 0 <= num <= den):
        raise ValueError(f"nms: bad IoU threshold {num} / {den} (integers, 0 <= num <= den, 1 <= den <= 2^16)")
    return num, den


@torch.no_grad()
def nms(box, label, num, den, per_label=False):
    """box int32 (P,4) xyxy with exclusive ends and label int32 (P), both in suppression order, on the device -> keep u8 (P): box
    j is suppressed by a KEPT box i < j (of its label, if per_label) when inter * den > num * union."""
    who = "nms"
    box = _lib.arg(box, torch.int32, (None, 4), who, "box")
    P = box.shape[0]
    num, den = _threshold((num, den))
    if P > MAX_NMS:
        raise ValueError(f"{who}: {P} boxes in one call (the limit is {MAX_NMS})")
    if per_label:
        label = _lib.arg(label, torch.int32, (P,), who, "label")
        _lib.on_gpu(who, label=label)
    _lib.on_gpu(who, box=box)
    words = (P + 63) // 64
    sup = torch.empty(P, words, dtype=torch.int64, device=box.device)
    _call("gpa_nms_matrix", box, label if per_label else None, P, num, den, 1 if per_label else 0, sup, _lib.stream_ptr())
    return nms_keep(sup)


@torch.no_grad()
def nms_keep(sup):
    """sup int64 (P, (P + 63) // 64) on the device, the suppression bits of gpa_nms_matrix (or of gpc_sup_bits, from mask IoUs) ->
    keep u8 (P): the greedy pass, gpa_nms_keep."""
    who = "nms_keep"
    sup = _lib.arg(sup, torch.int64, (None, None), who, "sup")
    P = sup.shape[0]
    if P > MAX_NMS or sup.shape[1] != (P + 63) // 64:
        raise ValueError(f"{who}: expected sup (P, (P + 63) // 64) with P <= {MAX_NMS}, got {tuple(sup.shape)}")
    _lib.on_gpu(who, sup=sup)
    keep = torch.empty(P, dtype=torch.uint8, device=sup.device)
    _call("gpa_nms_keep", sup, P, keep, _lib.stream_ptr())
    return keep


# ------------------------------------------------------------------------------------------------ the bank
def _crops_of(item):
    if isinstance(item, torch.Tensor):
        return item
    if isinstance(item, dict):
        return item["rgb"]
    return item.rgb


class DescriptorBank:
    """The descriptors of the onboarded objects: .q int32 (O, T, C) on the device, .labels the objects' category ids in bank order.
    add(label, crops): crops (T, 3, 224, 224) f32 on the device, or what holds them as "rgb" / .rgb -- the output of
    onboard.TemplateOnboarder, an item of onboard.RenderedTemplates or render.MeshTemplates.  Every object has the same number of
    templates (ValueError otherwise); a template whose descriptor is flagged (non-finite, zero norm) is a ValueError too."""

    def __init__(self, vit=None):
        self.vit = vit
        self.labels = []
        self._q = []

    def __len__(self):
        return len(self.labels)

    @property
    def q(self):
        if not self._q:
            raise ValueError("DescriptorBank: the bank is empty")
        return torch.stack(self._q)

    def add(self, label, crops):
        if self.vit is None:
            raise ValueError("DescriptorBank.add needs the ViT the bank was made for (a loaded bank is read-only without one)")
        label = int(label)
        if label in self.labels:
            raise ValueError(f"DescriptorBank: object {label} is in the bank already")
        crops = _crops_of(crops)
        if not (isinstance(crops, torch.Tensor) and crops.dim() == 4 and tuple(crops.shape[1:]) == (3, 224, 224)):
            raise ValueError(f"DescriptorBank: object {label}: expected crops (T, 3, 224, 224), got {tuple(getattr(crops, 'shape', ()))}")
        T = crops.shape[0]
        if T < 1 or (self._q and T != self._q[0].shape[0]):
            raise ValueError(f"DescriptorBank: object {label} has {T} templates, the bank's objects have {self._q[0].shape[0] if self._q else '>= 1'} "
                             "(objects with different template counts are out of scope)")
        q, status = self.vit.cls_descriptors(crops)
        flagged = torch.nonzero(status).flatten().tolist()
        if flagged:
            raise ValueError(f"DescriptorBank: object {label}: the descriptor of template {flagged[0]} is flagged (status {int(status[flagged[0]])}: "
                             "1 = not finite, 2 = zero norm)")
        self.labels.append(label)
        self._q.append(q)
        return self

    def save(self, path):
        """One .npz: q (O, T, C) int32, labels (O) int64, q_bits."""
        with open(path, "wb") as fh:
            np.savez(fh, q=self.q.cpu().numpy(), labels=np.asarray(self.labels, np.int64), q_bits=np.int64(Q_BITS))

    @classmethod
    def from_arrays(cls, q, labels, device="cuda", vit=None):
        """A bank from descriptors computed elsewhere: q int32 (O, T, C) within 2^20, labels (O)."""
        q, labels = np.asarray(q), np.asarray(labels)
        if q.dtype != np.int32 or q.ndim != 3 or 0 in q.shape or labels.shape != (q.shape[0],) or np.abs(q).max(initial=0) > 1 << Q_BITS:
            raise ValueError(f"DescriptorBank: expected q int32 (O, T, C) within 2^{Q_BITS} and labels (O), got {q.dtype} {q.shape} and {labels.shape}")
        if len(set(int(v) for v in labels)) != len(labels):
            raise ValueError("DescriptorBank: an object is in the bank twice")
        bank = cls(vit)
        bank.labels = [int(v) for v in labels]
        bank._q = list(torch.from_numpy(np.ascontiguousarray(q)).to(device))
        return bank

    @classmethod
    def load(cls, path, device="cuda", vit=None):
        with np.load(path) as z:
            if sorted(z.files) != ["labels", "q", "q_bits"] or int(z["q_bits"]) != Q_BITS:
                raise ValueError(f"DescriptorBank.load: {path} does not hold a bank (q, labels, q_bits = {Q_BITS})")
            q, labels = z["q"], z["labels"]
        return cls.from_arrays(q, labels, device, vit)


# ------------------------------------------------------------------------------------------------ the labeller
class ProposalLabeller:
    """Class-agnostic mask proposals -> labelled detections.

    vit: any vit.Dinov2ViT.  CNOS describes crops with the VANILLA DINOv2 checkpoint (dinov2_vitl14 as published), not with
    GigaPose's fine-tuned backbone: load the published weights into a Dinov2ViT of its own for this stage.  (No checkpoint is
    available to the tests; they use randomly initialised weights and prove plumbing, not accuracy.)
    bank: a DescriptorBank made with the same vit.  top_k: the templates an object's score is the mean of (CNOS: 5).  min_score:
    proposals below it are dropped.  nms_iou = (num, den): a kept box suppresses a later one when IoU > num / den, on integers.
    per_label: only boxes of one label suppress each other.  max_dets: at most this many detections per image, best first.
    nms_on: "box" (the default) compares the boxes; "mask" compares the masks themselves (detections.mask_nms: the same threshold,
    the same greedy pass, the IoU of the run-length masks; at most 2048 proposals above min_score per image).
    appearance: None (the default: the label rests on the class-token score alone, and libgigapose_appear.so is not loaded) or an
    appearance.PatchBank made with the same vit, holding the same labels in the same order as `bank` (ValueError otherwise).  With
    one, a proposal's crop is compared patch by patch with the best template of its label (bank row label * T + best_template): the
    dicts gain `semantic_score` (the class-token score) and `appearance_score` (the mean over the crop's valid patches of the best
    cosine among the template's valid patches), and `score` = (semantic + appearance) / 2 in float64 -- min_score, the NMS order
    and max_dets go by it, ties to the lower proposal index.  A proposal whose crop has no valid patch is dropped and counted in
    report["no_patch"].

    label(frames_u8, proposals) -> per image the list of CNOS dicts {bbox xywh, category_id, score, segmentation, best_template}
    (+ proposal: the index in the image's input list), best first; ingest.FrameIngest.__call__ takes them unchanged.  `report` counts what the last call dropped and why."""

    def __init__(self, vit, bank, top_k=5, min_score=0.5, nms_iou=(1, 4), per_label=False, max_dets=None, device="cuda", nms_on="box",
                 appearance=None):
        self.vit, self.bank = vit, bank
        if appearance is not None and list(appearance.labels) != list(bank.labels):
            raise ValueError(f"ProposalLabeller: the PatchBank holds the objects {list(appearance.labels)}, the DescriptorBank {list(bank.labels)} "
                             "(the same labels in the same order)")
        self.appearance = appearance
        self.top_k, self.min_score = int(top_k), float(min_score)
        if not 1 <= self.top_k <= MAX_K:
            raise ValueError(f"ProposalLabeller: top_k = {top_k} (1 to {MAX_K})")
        if self.min_score != self.min_score:
            raise ValueError("ProposalLabeller: min_score is NaN")
        self.nms_iou = _threshold(nms_iou)
        self.per_label = bool(per_label)
        if nms_on not in ("box", "mask"):
            raise ValueError(f"ProposalLabeller: nms_on must be 'box' or 'mask', got {nms_on!r}")
        self.nms_on = nms_on
        if max_dets is not None and int(max_dets) < 0:
            raise ValueError(f"ProposalLabeller: max_dets = {max_dets}")
        self.max_dets = None if max_dets is None else int(max_dets)
        self.device = torch.device(device)
        self.preprocess = RleDetectionPreprocessor(224)
        self.report = {}

    @staticmethod
    def host_batch(proposals, H, W):
        """Per-image proposal lists -> (segmentations, counts, offsets, image id (P) int32, given boxes xyxy int64 (P,4), which (P) bool,
        the index of each proposal in its image's list)."""
        segs, im_id, local, boxes, given = [], [], [], [], []
        for im, props in enumerate(proposals):
            for n, prop in enumerate(props):
                segs.append(prop["segmentation"])
                im_id.append(im)
                local.append(n)
                given.append(prop.get("bbox") is not None)
                boxes.append(prop["bbox"] if given[-1] else (0, 0, 0, 0))
        counts, offsets = pack_rle(segs, H, W)
        xyxy = xywh_to_xyxy_long(np.asarray(boxes, np.float32).reshape(-1, 4))
        return segs, counts, offsets, np.asarray(im_id, np.int32), xyxy, np.asarray(given, bool), local

    @torch.no_grad()
    def describe(self, frames_u8, proposals):
        """The device half up to the scores -> dict of host arrays (box int64 (P,4) xyxy, mstatus, dstatus, label, score,
        best_template, image) + "segs" + the device tensors "crops" and "q".  With a PatchBank also: the device tensors "tar_mask", "a" (limbs), "pstatus",
        "pvalid", "pcount", "pair_t" (the bank row of each proposal) and the host arrays "app_sum", "app_n", "app_status" (gpp_appearance's)."""
        if isinstance(frames_u8, np.ndarray):
            frames_u8 = torch.from_numpy(frames_u8)
        if not (isinstance(frames_u8, torch.Tensor) and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[1] == 3):
            raise ValueError("ProposalLabeller: expected u8 frames (n_img, 3, H, W)")
        n_img, _, H, W = frames_u8.shape
        if len(proposals) != n_img:
            raise ValueError(f"ProposalLabeller: {n_img} frames for {len(proposals)} proposal lists")
        segs, counts, offsets, im_id, given_xyxy, given, local = self.host_batch(proposals, H, W)
        if self.device.type != "cuda":
            raise _lib.GigaPoseHipError("ProposalLabeller needs a GPU device (no CPU fallback)")
        P, dev = len(segs), self.device
        frames = frames_u8.to(dev, non_blocking=True)
        counts_d, offsets_d = torch.from_numpy(counts).to(dev), torch.from_numpy(offsets).to(dev)
        (box_d, _, mstatus_d), lists = mask_boxes_and_lists(counts_d, offsets_d, H, W)
        box, mstatus = box_d.cpu().numpy().astype(np.int64), mstatus_d.cpu().numpy()
        box[given] = given_xyxy[given]                                  # a proposal's own box stands
        crop_box = box.copy()
        crop_box[mstatus != 0] = (0, 0, 1, 1)                           # an empty mask is dropped below: any box inside the frame does
        if self.appearance is None:
            crops = self.preprocess(frames, counts_d, offsets_d, crop_box, im_id)["tar_img"]
            q, dstatus = self.vit.cls_descriptors(crops)
        else:
            pre = self.preprocess(frames, counts_d, offsets_d, crop_box, im_id)
            crops = pre["tar_img"]
            patch = self.vit.cls_and_patch_descriptors(crops, pre["tar_mask"], occupancy=self.appearance.occupancy)
            q, dstatus = patch["q"], patch["status"]
        sc = scores(q, self.bank.q, self.top_k) if P else dict(label=torch.zeros(0, dtype=torch.int32), score=torch.zeros(0, dtype=torch.int64),
                                                               best_template=torch.zeros(0, dtype=torch.int32), kk=min(self.top_k, self.bank.q.shape[1]))
        host = {k: sc[k].cpu().numpy() for k in ("label", "score", "best_template")}
        out = dict(host, kk=sc["kk"], box=box, mstatus=mstatus, dstatus=dstatus.cpu().numpy(), image=im_id, segs=segs, crops=crops, q=q,
                   score_dev=sc["score"], n_img=n_img, local=local, lists=lists, HW=H * W)
        if self.appearance is not None:
            from . import appearance as app

            T = self.bank.q.shape[1]
            if P and (self.appearance.templates != T or self.appearance.a.shape[3] != q.shape[1]):
                raise ValueError(f"ProposalLabeller: the PatchBank has {self.appearance.templates} templates of {self.appearance.a.shape[3]} channels, "
                                 f"the DescriptorBank {T} of {q.shape[1]}")
            pair_t = (sc["label"].to(dev) * T + sc["best_template"].to(dev)).to(torch.int32)
            if P:
                res = app.appearance(patch["a"], patch["valid"], self.appearance.a, self.appearance.valid, torch.arange(P, dtype=torch.int32, device=dev), pair_t)
            else:
                res = dict(sum=torch.zeros(0, dtype=torch.int64), n=torch.zeros(0, dtype=torch.int32), status=torch.zeros(0, dtype=torch.int32))
            out.update(tar_mask=pre["tar_mask"], a=patch["a"], pstatus=patch["pstatus"], pvalid=patch["valid"], pcount=patch["count"], pair_t=pair_t,
                       app_sum=res["sum"].cpu().numpy(), app_n=res["n"].cpu().numpy(), app_status=res["status"].cpu().numpy())
        return out

    @torch.no_grad()
    def label(self, frames_u8, proposals):
        s = self.describe(frames_u8, proposals)
        P, dev = len(s["segs"]), self.device
        fscore = s["score"].astype(np.float64) / np.float64(s["kk"] * (1 << (2 * Q_BITS)))
        report = dict(proposals=P, empty_mask=0, flagged_descriptor=0, low_score=0, suppressed=0, over_max_dets=0, kept=0)
        empty, flagged = s["mstatus"] != 0, (s["mstatus"] == 0) & (s["dstatus"] != 0)
        semantic, order_key = fscore, None
        if self.appearance is not None:
            from . import appearance as app

            no_patch = ~empty & ~flagged & ((s["app_status"] & app.NO_QUERY_PATCH) != 0)
            appear = app.float_appearance(s["app_sum"], s["app_n"])
            fscore = (semantic + appear) / np.float64(2.0)                # the halving is exact
            report["no_patch"] = int(no_patch.sum())
            flagged = flagged | no_patch                                 # dropped alike; counted apart
            order_key = torch.from_numpy(fscore).to(dev) if P else None
        low = ~empty & ~flagged & (fscore < self.min_score)
        report.update(empty_mask=int(empty.sum()), flagged_descriptor=int(flagged.sum()) - report.get("no_patch", 0), low_score=int(low.sum()))
        alive = ~(empty | flagged | low)
        box32 = torch.from_numpy(s["box"].clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(dev) if P else None
        label32 = torch.from_numpy(s["label"]).to(dev) if P else None
        if self.nms_on == "mask" and P:
            from . import detections                                    # detections imports this module

            fg = detections.foreground(s["lists"], s["HW"])
        out = []
        for im in range(s["n_img"]):
            idx = np.flatnonzero(alive & (s["image"] == im))
            if len(idx) > MAX_NMS:
                raise ValueError(f"ProposalLabeller: image {im} has {len(idx)} proposals above min_score (the NMS takes {MAX_NMS}); raise min_score")
            dets = []
            if len(idx):
                idx_d = torch.from_numpy(idx).to(dev)
                key = s["score_dev"] if order_key is None else order_key
                order = torch.sort(key[idx_d], descending=True, stable=True).indices      # ties: the lower proposal index first
                idx_d = idx_d[order]
                if self.nms_on == "mask":
                    keep = detections.mask_nms(fg, idx_d, *self.nms_iou, label=label32 if self.per_label else None)
                else:
                    keep = nms(box32[idx_d].contiguous(), label32[idx_d].contiguous(), *self.nms_iou, per_label=self.per_label)
                kept = idx_d[keep.bool()].cpu().tolist()
                report["suppressed"] += len(idx) - len(kept)
                if self.max_dets is not None and len(kept) > self.max_dets:
                    report["over_max_dets"] += len(kept) - self.max_dets
                    kept = kept[:self.max_dets]
                for p in kept:
                    x0, y0, x1, y1 = (int(v) for v in s["box"][p])
                    dets.append(dict(bbox=[x0, y0, x1 - x0, y1 - y0], category_id=self.bank.labels[int(s["label"][p])], score=float(fscore[p]),
                                     segmentation=s["segs"][p], best_template=int(s["best_template"][p]), proposal=s["local"][p]))
                    if self.appearance is not None:
                        dets[-1].update(semantic_score=float(semantic[p]), appearance_score=float(appear[p]))
            report["kept"] += len(dets)
            out.append(dets)
        self.report = report
        return out
