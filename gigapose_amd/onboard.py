"""Templates in: the RGBA renders of an object (u8, as a PNG decoder yields them) -> the item GigaPose.set_template_data consumes,
with the boxes taken from the alpha channel and the crops normalised ON the GPU (libgigapose_onboard.so, C-ABI:
include/gigapose_onboard.h).

The reference does this on the CPU, one render at a time (TemplateData.load_template, src/custom_megapose/template_dataset.py:66-83:
PIL getbbox() and a float RGBA stack per object; TemplateSet.__getitem__, src/dataloader/template.py:55-81: CropResizePad and
normalize).  Here the u8 renders cross PCIe as they are (1.2 MB per 480 x 640 render) and two kernels do the rest:
gpo_alpha_boxes (getbbox on the alpha channel -- Pillow >= 10's default, alpha_only=True) and gpo_crop_templates (rgba / 255,
crop, (x - mean) / std on the colour; the mask is the cropped alpha / 255 with its 256 levels, and the colour is not multiplied by
it).  The results equal the reference's bit for bit (tests/test_gpu_onboard.py against tests/golden/onboard_templates.npz).

  alpha_boxes(rgba_u8)                 (N,H,W,4) u8 on the device -> int64 (N,4) xyxy on the device
  TemplateOnboarder                    renders (+ optional boxes) -> {"rgb", "mask", "M", "box"}
  load_renders(template_dir)           {view_id:06d}.png of one object -> u8 (N,H,W,4) numpy array
  RenderedTemplates                    drop-in for model.template_datasets[name]: item i has .rgb .mask .K .M .poses
Rendering is gigapose_amd/render.py's (MeshTemplates: mesh in, the same item out).  Out of scope here: pose files and the composition of poses (the caller passes what the reference's load_pose returns, in
bank order), template depth maps.  There is no CPU fallback: the kernels need the GPU, a missing library is an error.
"""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import torch

from . import _lib
from .crop import CLIP_MEAN, CLIP_STD
from .tensor_collection import PandasTensorCollection

MAX_TEMPLATES_PER_CALL = 65535                      # the grid's second dimension (gigapose_onboard.h: Limits)
TEMPLATE_K = ((572.4114, 0.0, 320.0), (0.0, 573.57043, 240.0), (0.0, 0.0, 1.0))   # template_dataset.py:194-196
_onboard = _lib.SideLibrary("libgigapose_onboard.so", "gpo")
ONBOARD_LIB_PATH, lib, _call = _onboard.path, _onboard.lib, _onboard.call


def _device_renders(rgba_u8, who):
    if not (isinstance(rgba_u8, torch.Tensor) and rgba_u8.is_cuda):
        raise _lib.GigaPoseHipError(f"{who} needs the renders on the GPU (no CPU fallback)")
    if not (rgba_u8.dtype == torch.uint8 and rgba_u8.dim() == 4 and rgba_u8.shape[3] == 4):
        raise ValueError(f"{who}: expected u8 renders (N, H, W, 4), got {rgba_u8.dtype} {tuple(rgba_u8.shape)}")
    rgba_u8 = rgba_u8.contiguous()
    if rgba_u8.storage_offset() % 4:                 # a byte view at an odd offset (allocations start aligned): one pixel must be one aligned word
        rgba_u8 = rgba_u8.clone()
    return rgba_u8


def _alpha_boxes(rgba_u8, boxes, err):
    """boxes (N,4) int64 and err (chunks,) int32 on the device; chunk c of 65535 renders reports into err[c]."""
    N, H, W, _ = rgba_u8.shape
    for c, a, b in _lib.chunked(N, MAX_TEMPLATES_PER_CALL):
        _call("gpo_alpha_boxes", rgba_u8[a:b], b - a, H, W, boxes[a:b], err[c:c + 1], _lib.stream_ptr())


@torch.no_grad()
def alpha_boxes(rgba_u8):
    """PIL getbbox() of every render's alpha channel: (N,H,W,4) u8 on the device -> int64 (N,4) xyxy on the device.
    Raises ValueError, naming the template, when one is fully transparent (getbbox() returns None there)."""
    rgba_u8 = _device_renders(rgba_u8, "alpha_boxes")
    N = rgba_u8.shape[0]
    boxes = torch.empty(N, 4, dtype=torch.int64, device=rgba_u8.device)
    err = torch.zeros(max(1, -(-N // MAX_TEMPLATES_PER_CALL)), dtype=torch.int32, device=rgba_u8.device)
    _alpha_boxes(rgba_u8, boxes, err)
    bad = _lib.first_bad(err.tolist(), MAX_TEMPLATES_PER_CALL)
    if bad is not None:
        raise ValueError(f"alpha_boxes: template {bad} is fully transparent")
    return boxes


class TemplateOnboarder:
    """renders u8 (N,H,W,4) on the device -> {"rgb" (N,3,T,T), "mask" (N,T,T), "M" (N,3,3), "box" (N,4) int64}: what
    TemplateSet.__getitem__ (src/dataloader/template.py:64-70) computes from load_template's rgba and box, bit for bit."""

    def __init__(self, target_size=224, mean=CLIP_MEAN, std=CLIP_STD):
        self.target_size = target_size
        self._mean = (ctypes.c_float * 3)(*mean)
        self._std = (ctypes.c_float * 3)(*std)

    @torch.no_grad()
    def __call__(self, rgba_u8, boxes=None, out=None):
        """`boxes` (N,4) xyxy replaces the alpha boxes; `out` = {"rgb", "mask", "M"} are buffers to write into (a bad template
        leaves its slices of them untouched).  One host synchronisation: the read of the error flags."""
        rgba_u8 = _device_renders(rgba_u8, "TemplateOnboarder")
        dev = rgba_u8.device
        N, H, W, _ = rgba_u8.shape
        T = self.target_size
        shapes = {"rgb": (N, 3, T, T), "mask": (N, T, T), "M": (N, 3, 3)}
        if out is None:
            out = {k: torch.empty(s, device=dev) for k, s in shapes.items()}
        for k, s in shapes.items():
            t = out[k]
            if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == s and t.is_contiguous()):
                raise ValueError(f"TemplateOnboarder: out[{k!r}] must be a contiguous float32 tensor {s} on the GPU")
        chunks = max(1, -(-N // MAX_TEMPLATES_PER_CALL))
        err = torch.zeros(2, chunks, dtype=torch.int32, device=dev)     # [0]: the alpha boxes' flags, [1]: the crops'
        given = boxes is not None
        if given:
            boxes = torch.as_tensor(boxes).to(device=dev, dtype=torch.int64).contiguous()
            if tuple(boxes.shape) != (N, 4):
                raise ValueError(f"TemplateOnboarder: expected boxes ({N}, 4), got {tuple(boxes.shape)}")
        else:
            boxes = torch.empty(N, 4, dtype=torch.int64, device=dev)
            _alpha_boxes(rgba_u8, boxes, err[0])
        for c, a, b in _lib.chunked(N, MAX_TEMPLATES_PER_CALL):
            _call("gpo_crop_templates", rgba_u8[a:b], boxes[a:b], b - a, H, W, T, self._mean, self._std, out["rgb"][a:b], out["mask"][a:b], out["M"][a:b],
                  err[1, c:c + 1], _lib.stream_ptr())
        no_alpha, no_crop = err.tolist()
        bad = _lib.first_bad(no_alpha, MAX_TEMPLATES_PER_CALL)
        if bad is not None:
            raise ValueError(f"TemplateOnboarder: template {bad} is fully transparent (PIL getbbox() returns None for it)")
        bad = _lib.first_bad(no_crop, MAX_TEMPLATES_PER_CALL)
        if bad is not None:
            why = "has an empty / out-of-frame box, or its " if given else "has a "
            raise ValueError(f"TemplateOnboarder: template {bad} {why}box scales to an empty crop (the short side times "
                             f"{T} / the long side is below one pixel)")
        return {"rgb": out["rgb"], "mask": out["mask"], "M": out["M"], "box": boxes}


_VIEW = re.compile(r"^(\d{6})\.png$")


def load_renders(template_dir, num_templates=None):
    """The renders of one object in the reference's layout, `{view_id:06d}.png` (template_dataset.py:66-67), read through PIL ->
    u8 (N,H,W,4), ordered by view id.  `num_templates=None` takes every view the directory holds.  Raises ValueError on a
    missing view, on a file that is not RGBA and on mixed sizes."""
    from PIL import Image

    template_dir = os.fspath(template_dir)
    if num_templates is None:
        ids = sorted(int(m.group(1)) for m in map(_VIEW.match, os.listdir(template_dir)) if m)
        if not ids:
            raise ValueError(f"load_renders: no {{view_id:06d}}.png in {template_dir}")
        num_templates = ids[-1] + 1
    views = []
    for view_id in range(int(num_templates)):
        path = os.path.join(template_dir, f"{view_id:06d}.png")
        if not os.path.exists(path):
            raise ValueError(f"load_renders: view {view_id} is missing ({path})")
        with Image.open(path) as im:
            if im.mode != "RGBA":
                raise ValueError(f"load_renders: {path} has mode {im.mode}, not RGBA (the box and the mask come from the alpha channel)")
            a = np.array(im)
        if views and a.shape != views[0].shape:
            raise ValueError(f"load_renders: {path} is {a.shape[1]} x {a.shape[0]}, view 0 is {views[0].shape[1]} x {views[0].shape[0]}")
        views.append(a)
    return np.stack(views) if views else np.zeros((0, 0, 0, 4), np.uint8)


class RenderedTemplates:
    """Drop-in for `model.template_datasets[name]` (the reference's TemplateSet, src/dataloader/template.py:17-81): item i is a
    PandasTensorCollection with .rgb (N,3,T,T) .mask (N,T,T) .K (3,3) .M (N,3,3) .poses (N,4,4) on the device.

    objects: list of (renders, poses) -- renders a u8 array / tensor (N,H,W,4) or a directory for load_renders, poses (N,4,4)
    as the reference's load_pose returns them, in bank order (LM-O's index -> id mapping is the caller's).  K defaults to the
    reference's template intrinsics.  The u8 renders stay on the HOST (pinned when a GPU is there) and every __getitem__ uploads
    and crops them again: set_template_data asks for an item up to three times, and the float crops of 40 objects must not
    become resident."""

    def __init__(self, objects, K=None, device="cuda", target_size=224):
        self.device = torch.device(device)
        self.onboard = TemplateOnboarder(target_size)
        self.K = torch.as_tensor(np.asarray(TEMPLATE_K if K is None else K, dtype=np.float32).reshape(3, 3))
        self._renders, self._poses = [], []
        for o, (renders, poses) in enumerate(objects):
            if isinstance(renders, (str, os.PathLike)):
                renders = load_renders(renders)
            r = torch.as_tensor(renders)
            if isinstance(poses, torch.Tensor):
                poses = poses.detach().cpu().numpy()
            p = torch.as_tensor(np.asarray(poses, dtype=np.float32))
            if not (r.dtype == torch.uint8 and r.dim() == 4 and r.shape[3] == 4):
                raise ValueError(f"RenderedTemplates: object {o}: expected u8 renders (N, H, W, 4), got {r.dtype} {tuple(r.shape)}")
            if tuple(p.shape) != (r.shape[0], 4, 4):
                raise ValueError(f"RenderedTemplates: object {o}: {r.shape[0]} renders but poses {tuple(p.shape)}")
            r = r.cpu().contiguous()
            self._renders.append(r.pin_memory() if torch.cuda.is_available() else r)
            self._poses.append(p)

    def __len__(self):
        return len(self._renders)

    @torch.no_grad()
    def __getitem__(self, i):
        if self.device.type != "cuda":
            raise _lib.GigaPoseHipError("RenderedTemplates needs a GPU device (no CPU fallback)")
        try:
            out = self.onboard(self._renders[i].to(self.device, non_blocking=True))
        except ValueError as e:
            raise ValueError(f"RenderedTemplates: object {i}: {e}") from None
        return PandasTensorCollection(infos=pd.DataFrame(), K=self.K.to(self.device), rgb=out["rgb"], mask=out["mask"], M=out["M"],
                                      poses=self._poses[i].to(self.device))
