"""The appearance score of a mask proposal: the patch-level companion of the class-token score of proposals.py
(libgigapose_appear.so, C-ABI: include/gigapose_appear.h).

CNOS's successors (the instance segmentation stage of SAM-6D) take, for every foreground patch of a proposal's crop, its best
cosine match among the foreground patches of the object's best template, average the matches, and average that with the
class-token score.  Here: the 256 patch tokens of the ViT after the final LayerNorm, L2-normalised and quantised to 2^-20 as the
class token is, each component stored as three int8 limbs; the patches a crop's mask occupies; per (proposal, template) pair the
256 x 256 x C exact integer products on gfx950's int8 MFMA, the masked maximum with the first-j rule and the int64 sum.  Every
decision is taken on integers; gigapose_testing/appear_ref.py restates the arithmetic and agrees bit for bit.

  patch_descriptors(x, ...)            patch tokens (any strides) -> (a int8 (3, B, 256, C), status (B, 256))   gpp_patch_descriptors
  patch_valid(mask, num, den)          crop masks (B, 224, 224) -> valid u8 (B, 256), count (B) (+ set)          gpp_patch_valid
  appearance(qa, q_valid, ta, ...)     pairs -> sum int64, n, status (+ best, arg)                               gpp_appearance
  float_appearance(sum, n)             sum / (n * 2^40) in float64
  q_to_limbs(q) / limbs_to_q(a)        the balanced base-128 digits on the host (numpy)
  PatchBank                            the limbs and valid patches of the onboarded objects' templates
A bank holds 3 bytes per value: 3 * 256 * C bytes per template, 33 MB per object at 42 templates of ViT-L (C = 1024), 127 MB at
162.  Out of scope: CNOS's visibility / geometric score, objects with different template counts.  There is no CPU fallback: the
kernels need the GPU, a missing library is an error.  No checkpoint and no real data have been through this stage: the tests prove
plumbing and arithmetic, not accuracy.
"""
import numpy as np
import torch

from . import _lib

PATCHES, CELL, CROP = 256, 14, 224
Q_BITS = 20
MAX_C, MAX_ROWS, MAX_PAIRS = 2048, 1 << 20, 65535
NON_FINITE, ZERO_NORM = 1, 2                                # status bits of patch_descriptors (GPP_NON_FINITE, GPP_ZERO_NORM)
BAD_INDEX, NO_QUERY_PATCH, NO_TEMPLATE_PATCH = 1, 2, 4      # status bits of appearance
_appear = _lib.SideLibrary("libgigapose_appear.so", "gpp")
APPEAR_LIB_PATH, lib, _call = _appear.path, _appear.lib, _appear.call


# ------------------------------------------------------------------------------------------------ limbs on the host
def q_to_limbs(q):
    """q integers (..) in [-2^20, 2^20] -> int8 (3, ..): q = a0 + 128 a1 + 16384 a2 with a0, a1 in [-64, 63], a2 in [-64, 64]."""
    q = np.asarray(q)
    if q.dtype.kind not in "iu" or np.abs(q.astype(np.int64)).max(initial=0) > 1 << Q_BITS:
        raise ValueError(f"q_to_limbs: expected integers within 2^{Q_BITS}")
    q = q.astype(np.int64)
    a0 = ((q + 64) & 127) - 64
    q1 = (q - a0) >> 7
    a1 = ((q1 + 64) & 127) - 64
    return np.stack([a0, a1, (q1 - a1) >> 7]).astype(np.int8)


def limbs_to_q(a):
    """int8 (3, ..) -> q int32 (..)."""
    a = np.asarray(a)
    if a.dtype != np.int8 or a.ndim < 1 or a.shape[0] != 3:
        raise ValueError(f"limbs_to_q: expected int8 (3, ..), got {a.dtype} {a.shape}")
    a = a.astype(np.int32)
    return a[0] + 128 * a[1] + 16384 * a[2]


def _threshold(occupancy):
    num, den = (int(v) for v in occupancy)
    if not (1 <= den <= 65536 and 0 <= num <= den):
        raise ValueError(f"patch_valid: bad threshold {num} / {den} (integers, 0 <= num <= den, 1 <= den <= 2^16)")
    return num, den


# ------------------------------------------------------------------------------------------------ the kernels, one wrapper each
@torch.no_grad()
def patch_descriptors(x, crop_stride, token_stride, channel_stride, gamma, beta, eps, B, C, offset=0):
    """x: an f32 tensor on the device whose storage holds value c of patch n of crop b at element offset + b * crop_stride + n *
    token_stride + c * channel_stride from x's first element (offset: C for the contiguous (B, 257, C), 1 for the ViT workspace's
    channel-major view -- the class token is skipped) -> (a int8 (3, B, 256, C), status int32 (B, 256))."""
    who = "patch_descriptors"
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32):
        raise ValueError(f"{who}: x must be a float32 tensor")
    B, C, offset = int(B), int(C), int(offset)
    crop_stride, token_stride, channel_stride = int(crop_stride), int(token_stride), int(channel_stride)
    if not (C >= 64 and C <= MAX_C and C % 64 == 0):
        raise ValueError(f"{who}: C = {C} channels (a multiple of 64, 64 to {MAX_C})")
    if B < 0 or B > MAX_ROWS or offset < 0 or crop_stride <= 0 or token_stride <= 0 or channel_stride <= 0:
        raise ValueError(f"{who}: bad sizes B = {B}, offset {offset}, strides {crop_stride}, {token_stride}, {channel_stride}")
    if B and offset + (B - 1) * crop_stride + (PATCHES - 1) * token_stride + (C - 1) * channel_stride >= x.numel():
        raise ValueError(f"{who}: the strides leave x ({x.numel()} elements)")
    gamma, beta = _lib.arg(gamma, torch.float32, (C,), who, "gamma"), _lib.arg(beta, torch.float32, (C,), who, "beta")
    _lib.on_gpu(who, x=x, gamma=gamma, beta=beta)
    if not x.is_contiguous():
        raise ValueError(f"{who}: x is not contiguous (the strides are passed, not taken from the tensor)")
    a = torch.empty(3, B, PATCHES, C, dtype=torch.int8, device=x.device)
    status = torch.empty(B, PATCHES, dtype=torch.int32, device=x.device)
    _call("gpp_patch_descriptors", x.view(-1)[offset:] if B else x, crop_stride, token_stride, channel_stride, gamma, beta, eps, B, C, a, status,
          _lib.stream_ptr())
    return a, status


@torch.no_grad()
def patch_valid(mask, num=1, den=2, want_set=False):
    """mask f32 (B, 224, 224) on the device (a crop's tar_mask) -> (valid u8 (B, 256), count int32 (B)) (+ set u8 (B, 256) with
    want_set): patch n = 16 * (y / 14) + (x / 14) is valid iff more than num / den of its 196 pixels exceed 0.5."""
    who = "patch_valid"
    mask = _lib.arg(mask, torch.float32, (None, CROP, CROP), who, "mask")
    num, den = _threshold((num, den))
    B = mask.shape[0]
    if B > MAX_ROWS:
        raise ValueError(f"{who}: {B} crops in one call (the limit is {MAX_ROWS})")
    _lib.on_gpu(who, mask=mask)
    valid = torch.empty(B, PATCHES, dtype=torch.uint8, device=mask.device)
    count = torch.empty(B, dtype=torch.int32, device=mask.device)
    pixels = torch.empty(B, PATCHES, dtype=torch.uint8, device=mask.device) if want_set else None
    _call("gpp_patch_valid", mask, B, num, den, valid, count, pixels, _lib.stream_ptr())
    return (valid, count, pixels) if want_set else (valid, count)


@torch.no_grad()
def appearance(qa, q_valid, ta, t_valid, qi, ti, want=()):
    """qa int8 (3, Bq, 256, C) + q_valid u8 (Bq, 256): the query crops; ta int8 (3, R, 256, C) + t_valid u8 (R, 256): the bank's rows;
    qi, ti int32 (P): the pairs, all on the device -> dict(sum int64 (P), n int32 (P), status int32 (P)): include/gigapose_appear.h's
    gpp_appearance.  want: "best" (int64 (P, 256)) and / or "arg" (int32 (P, 256)) add those tensors.  More than 65535 pairs go in
    several calls."""
    who = "appearance"
    for what, t in (("qa", qa), ("ta", ta)):
        if not (isinstance(t, torch.Tensor) and t.dim() == 4):
            raise ValueError(f"{who}: {what} must be a (3, rows, 256, C) tensor")
    C = qa.shape[3]
    qa, ta = _lib.arg(qa, torch.int8, (3, None, PATCHES, C), who, "qa"), _lib.arg(ta, torch.int8, (3, None, PATCHES, C), who, "ta")
    Bq, R = qa.shape[1], ta.shape[1]
    q_valid = _lib.arg(q_valid, torch.uint8, (Bq, PATCHES), who, "q_valid")
    t_valid = _lib.arg(t_valid, torch.uint8, (R, PATCHES), who, "t_valid")
    qi = _lib.arg(qi, torch.int32, (None,), who, "qi")
    P = qi.shape[0]
    ti = _lib.arg(ti, torch.int32, (P,), who, "ti")
    if not (1 <= Bq <= MAX_ROWS and 1 <= R <= MAX_ROWS and C >= 64 and C <= MAX_C and C % 64 == 0):
        raise ValueError(f"{who}: bad sizes Bq = {Bq}, R = {R}, C = {C} (1 <= Bq, R <= 2^20, C a multiple of 64, 64 to {MAX_C})")
    unknown = set(want) - {"best", "arg"}
    if unknown:
        raise ValueError(f"{who}: want takes 'best' and 'arg', got {sorted(unknown)}")
    _lib.on_gpu(who, qa=qa, q_valid=q_valid, ta=ta, t_valid=t_valid, qi=qi, ti=ti)
    dev = qa.device
    out = dict(sum=torch.empty(P, dtype=torch.int64, device=dev), n=torch.empty(P, dtype=torch.int32, device=dev),
               status=torch.empty(P, dtype=torch.int32, device=dev))
    if "best" in want:
        out["best"] = torch.empty(P, PATCHES, dtype=torch.int64, device=dev)
    if "arg" in want:
        out["arg"] = torch.empty(P, PATCHES, dtype=torch.int32, device=dev)
    for _, a, b in _lib.chunked(P, MAX_PAIRS):
        _call("gpp_appearance", qa, q_valid, Bq, ta, t_valid, R, C, qi[a:b], ti[a:b], b - a, out["sum"][a:b], out["n"][a:b], out["status"][a:b],
              out["best"][a:b] if "best" in want else None, out["arg"][a:b] if "arg" in want else None, _lib.stream_ptr())
    return out


def float_appearance(total, n):
    """The int64 sums as float64 mean cosines: sum / (n * 2^40), one correctly rounded division; a pair without patches (n = 0) gives 0."""
    if isinstance(total, torch.Tensor):
        n64 = n.to(torch.float64)
        return torch.where(n64 > 0, total.to(torch.float64) / (n64.clamp(min=1.0) * float(1 << (2 * Q_BITS))), torch.zeros_like(n64))
    n64 = np.asarray(n, np.int64).astype(np.float64)
    return np.where(n64 > 0, np.asarray(total, np.int64).astype(np.float64) / (np.maximum(n64, 1.0) * np.float64(1 << (2 * Q_BITS))), 0.0)


# ------------------------------------------------------------------------------------------------ the bank
def _field(item, name):
    if isinstance(item, dict):
        return item[name]
    return getattr(item, name)


class PatchBank:
    """The patch descriptors of the onboarded objects: .a int8 (3, O * T, 256, C) and .valid u8 (O * T, 256) on the device (row o * T
    + t is template t of object o), .labels the objects' category ids in bank order, .templates = T.
    add(label, item): item holds the crops (T, 3, 224, 224) as "rgb" / .rgb and their masks (T, 224, 224) as "mask" / .mask -- the
    output of onboard.TemplateOnboarder, an item of onboard.RenderedTemplates or render.MeshTemplates; or add(label, crops, mask).
    Every object has the same number of templates (ValueError otherwise); a template with no valid patch is a ValueError that names
    it.  occupancy = (num, den): a patch is valid when more than num / den of its pixels lie on the mask.
    Size: 3 bytes per value, 768 * C bytes per template -- 33 MB per object at 42 templates of ViT-L, 127 MB at 162."""

    def __init__(self, vit=None, occupancy=(1, 2)):
        self.vit = vit
        self.occupancy = _threshold(occupancy)
        self.labels = []
        self._a, self._valid = [], []
        self._cat = None

    def __len__(self):
        return len(self.labels)

    @property
    def templates(self):
        if not self._a:
            raise ValueError("PatchBank: the bank is empty")
        return self._a[0].shape[1]

    def _joined(self):
        if not self._a:
            raise ValueError("PatchBank: the bank is empty")
        if self._cat is None:
            T = self.templates
            a, valid = torch.cat(self._a, dim=1), torch.cat(self._valid, dim=0)
            self._a = [a[:, o * T:(o + 1) * T] for o in range(len(self.labels))]          # views: the bank is held once
            self._valid = [valid[o * T:(o + 1) * T] for o in range(len(self.labels))]
            self._cat = (a, valid)
        return self._cat

    @property
    def a(self):
        return self._joined()[0]

    @property
    def valid(self):
        return self._joined()[1]

    def add(self, label, item, mask=None):
        if self.vit is None:
            raise ValueError("PatchBank.add needs the ViT the bank was made for (a loaded bank is read-only without one)")
        label = int(label)
        if label in self.labels:
            raise ValueError(f"PatchBank: object {label} is in the bank already")
        crops = item if isinstance(item, torch.Tensor) else _field(item, "rgb")
        mask = mask if mask is not None or isinstance(item, torch.Tensor) else _field(item, "mask")
        if not (isinstance(crops, torch.Tensor) and crops.dim() == 4 and tuple(crops.shape[1:]) == (3, CROP, CROP)):
            raise ValueError(f"PatchBank: object {label}: expected crops (T, 3, 224, 224), got {tuple(getattr(crops, 'shape', ()))}")
        T = crops.shape[0]
        if not (isinstance(mask, torch.Tensor) and tuple(mask.shape) == (T, CROP, CROP)):
            raise ValueError(f"PatchBank: object {label}: expected masks ({T}, 224, 224), got {tuple(getattr(mask, 'shape', ()))}")
        if T < 1 or (self._a and T != self.templates):
            raise ValueError(f"PatchBank: object {label} has {T} templates, the bank's objects have {self.templates if self._a else '>= 1'} "
                             "(objects with different template counts are out of scope)")
        d = self.vit.cls_and_patch_descriptors(crops, mask, occupancy=self.occupancy)
        empty = torch.nonzero(d["count"] == 0).flatten().tolist()
        if empty:
            raise ValueError(f"PatchBank: object {label}: template {empty[0]} has no valid patch (no patch with more than "
                             f"{self.occupancy[0]} / {self.occupancy[1]} of its pixels on the mask)")
        self.labels.append(label)
        self._a.append(d["a"])
        self._valid.append(d["valid"])
        self._cat = None
        return self

    def save(self, path):
        """One .npz: a (3, O, T, 256, C) int8, valid (O, T, 256) uint8, labels (O) int64, q_bits."""
        O, T = len(self.labels), self.templates
        a, valid = self.a.cpu().numpy(), self.valid.cpu().numpy()
        with open(path, "wb") as fh:
            np.savez(fh, a=a.reshape(3, O, T, PATCHES, a.shape[-1]), valid=valid.reshape(O, T, PATCHES), labels=np.asarray(self.labels, np.int64),
                     q_bits=np.int64(Q_BITS))

    @classmethod
    def from_arrays(cls, a, valid, labels, device="cuda", vit=None, occupancy=(1, 2)):
        """A bank from limbs computed elsewhere: a int8 (3, O, T, 256, C) within the limb ranges, valid uint8 (O, T, 256) with a valid
        patch in every template, labels (O)."""
        a, valid, labels = np.asarray(a), np.asarray(valid), np.asarray(labels)
        if (a.dtype != np.int8 or a.ndim != 5 or a.shape[0] != 3 or a.shape[3] != PATCHES or 0 in a.shape or valid.dtype != np.uint8
                or valid.shape != a.shape[1:4] or labels.shape != (a.shape[1],)):
            raise ValueError(f"PatchBank: expected a int8 (3, O, T, 256, C), valid uint8 (O, T, 256) and labels (O), got {a.dtype} {a.shape}, "
                             f"{valid.dtype} {valid.shape} and {labels.shape}")
        C = a.shape[4]
        if C % 64 or C > MAX_C:
            raise ValueError(f"PatchBank: C = {C} channels (a multiple of 64, 64 to {MAX_C})")
        if a[:2].min() < -64 or a[:2].max() > 63 or a[2].min() < -64 or a[2].max() > 64:
            raise ValueError("PatchBank: a limb leaves its range (a0, a1 in [-64, 63], a2 in [-64, 64])")
        if len(set(int(v) for v in labels)) != len(labels):
            raise ValueError("PatchBank: an object is in the bank twice")
        empty = np.argwhere(~(valid != 0).any(axis=2))
        if len(empty):
            raise ValueError(f"PatchBank: object {int(labels[empty[0][0]])}: template {int(empty[0][1])} has no valid patch")
        bank = cls(vit, occupancy)
        O, T = valid.shape[:2]
        bank.labels = [int(v) for v in labels]
        a_d = torch.from_numpy(np.ascontiguousarray(a.reshape(3, O * T, PATCHES, C))).to(device)
        v_d = torch.from_numpy(np.ascontiguousarray((valid != 0).astype(np.uint8).reshape(O * T, PATCHES))).to(device)
        bank._a, bank._valid = [a_d[:, o * T:(o + 1) * T] for o in range(O)], [v_d[o * T:(o + 1) * T] for o in range(O)]
        bank._cat = (a_d, v_d)
        return bank

    @classmethod
    def load(cls, path, device="cuda", vit=None, occupancy=(1, 2)):
        with np.load(path) as z:
            if sorted(z.files) != ["a", "labels", "q_bits", "valid"] or int(z["q_bits"]) != Q_BITS:
                raise ValueError(f"PatchBank.load: {path} does not hold a patch bank (a, valid, labels, q_bits = {Q_BITS})")
            a, valid, labels = z["a"], z["valid"], z["labels"]
        return cls.from_arrays(a, valid, labels, device, vit, occupancy)
