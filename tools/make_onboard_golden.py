"""Writes tests/golden/onboard_templates.npz: what the UNMODIFIED reference makes of the renders of
gigapose_testing.renders.golden_renders -- the box of every render by PIL's getbbox() as TemplateData.load_template takes it
(src/custom_megapose/template_dataset.py:76), rgba / 255 as load_set_of_templates stacks it (:103-109), CropResizePad
(src/utils/crop.py, imported from the reference tree where it lies through oracle/ref_shim.py) and, as TemplateSet.__getitem__
does (src/dataloader/template.py:67-70), the normalisation of the colour channels (torchvision Normalize is not installed;
restated as its documented `(x - mean) / std`, as oracle/make_goldens.py:gen_crop does).
Run once where the reference tree exists; no GPU test reads that tree, they read this file.

Stored: seed, boxes (8,4) int64, rgb (8,3,224,224), mask (8,224,224), M (8,3,3) and the checksum of the input renders."""
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_testing import renders  # noqa: E402
from gigapose_testing import synthetic as syn  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.crop_numpy import CLIP_MEAN, CLIP_STD  # noqa: E402


def reference_templates(rgba_u8, target=224):
    """rgba_u8 (N,H,W,4) -> dict(boxes, rgb, mask, M) as numpy arrays, computed by PIL and the reference's CropResizePad."""
    ref_shim.install()
    from src.utils.crop import CropResizePad

    boxes, stack = [], []
    for view in rgba_u8:
        box = Image.fromarray(view).getbbox()                  # load_template: rgba.getbbox()
        boxes.append(torch.from_numpy(np.array(box)).long())
        stack.append(torch.from_numpy(view / 255).float())             # load_set_of_templates
    rgba = torch.stack(stack).permute(0, 3, 1, 2)
    boxes = torch.stack(boxes)
    out = CropResizePad(target_size=target)(boxes, images=rgba)
    mean = torch.tensor(CLIP_MEAN).view(3, 1, 1)
    std = torch.tensor(CLIP_STD).view(3, 1, 1)
    rgb = (out["images"][:, :3] - mean) / std
    return dict(boxes=boxes.numpy(), rgb=rgb.numpy(), mask=out["images"][:, -1].contiguous().numpy(), M=out["M"].numpy())


def main():
    rgba = renders.golden_renders(renders.GOLDEN_SEED)
    ref = reference_templates(rgba)
    out = os.path.join(ROOT, "tests", "golden", "onboard_templates.npz")
    np.savez_compressed(out, seed=renders.GOLDEN_SEED, input_checksum=np.asarray(syn.checksum(rgba)), **ref)
    print(out, os.path.getsize(out), "bytes;", len(rgba), "renders; boxes", ref["boxes"].tolist())


if __name__ == "__main__":
    main()
