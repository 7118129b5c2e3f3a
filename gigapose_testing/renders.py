"""Deterministic synthetic RGBA renders for the onboarding tests (gigapose_amd/onboard.py), the golden generator
tools/make_onboard_golden.py and tools/probe_onboard.py.  numpy RandomState streams only, as synthetic.py.

A render is what np.array(PIL image) of a template PNG is: u8 (H,W,4), interleaved.  The colour is a smooth field that is
non-zero EVERYWHERE, also where alpha is 0, so a box taken from any channel but alpha is the full frame and wrong.  The alpha
channel is a gradient (1..255: the mask has 256 levels) over an ellipse inscribed in a requested box, and the four pixels that
make the box what it is -- leftmost, topmost, rightmost, bottommost -- carry alpha 1, 3, 7 and 255: a test of `alpha > 0` that
looks at a threshold, a sign bit or the low bits only misses one of them.
"""
import types

import numpy as np

from oracle import crop_numpy

from . import synthetic as syn


def colour_field(rs, H, W):
    """(H,W,3) u8 in 1..255: a sum of three plane waves per channel."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((H, W, 3), np.uint8)
    for c in range(3):
        f = np.zeros((H, W))
        for _ in range(3):
            kx, ky = rs.uniform(-0.12, 0.12, 2)
            f += np.cos(kx * xx + ky * yy + rs.uniform(0, 2 * np.pi))
        out[..., c] = np.clip(np.rint(128 + 40 * f), 1, 255).astype(np.uint8)
    return out


def render_with_box(rs, H, W, box):
    """One render whose alpha box is exactly `box` = (x0, y0, x1, y1), 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H."""
    x0, y0, x1, y1 = (int(v) for v in box)
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H, box
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[..., :3] = colour_field(rs, H, W)
    alpha = np.zeros((H, W), np.uint8)
    w, h = x1 - x0, y1 - y0
    if w > 2 and h > 2:   # an ellipse strictly inside the box, alpha a gradient over 1..255
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        cx, cy = x0 + (w - 1) / 2.0, y0 + (h - 1) / 2.0
        inside = ((xx - cx) / ((w - 2) / 2.0)) ** 2 + ((yy - cy) / ((h - 2) / 2.0)) ** 2 <= 1.0
        inside &= (xx > x0) & (xx < x1 - 1) & (yy > y0) & (yy < y1 - 1)
        grad = 1 + ((xx - x0) * 7 + (yy - y0) * 13) % 255
        alpha[inside] = grad[inside].astype(np.uint8)
    ym, xm = y0 + h // 2, x0 + w // 2
    alpha[ym, x0] = 1            # the four extreme pixels; on a box of one or two pixels they coincide and the last value stays
    alpha[y0, xm] = 3
    alpha[y0 + (h - 1) // 2, x1 - 1] = 7
    alpha[y1 - 1, x0 + (w - 1) // 2] = 255
    rgba[..., 3] = alpha
    return rgba


def renders_with_boxes(seed, H, W, boxes):
    rs = np.random.RandomState(seed)
    return np.stack([render_with_box(rs, H, W, b) for b in boxes])


def alpha_boxes_numpy(rgba):
    """PIL getbbox() of the alpha channel in numpy: (N,H,W,4) u8 -> int64 (N,4) xyxy; a fully transparent render gives 0,0,0,0."""
    rgba = np.asarray(rgba)
    out = np.zeros((rgba.shape[0], 4), np.int64)
    for n, a in enumerate(rgba[..., 3] > 0):
        cols, rows = np.flatnonzero(a.any(axis=0)), np.flatnonzero(a.any(axis=1))
        if len(cols):
            out[n] = (cols[0], rows[0], cols[-1] + 1, rows[-1] + 1)
    return out


# The box classes of CropResizePad at 480 x 640, target 224: every branch of the source-index arithmetic (gp_crop_geom.h)
BOX_CLASSES_480x640 = [
    ("224 x 224: both resizes are the identity", (200, 100, 424, 324)),
    ("112 x 112: the first resize is dst >> 1", (300, 200, 412, 312)),
    ("448 x 448, centred: scale 1/2", (96, 16, 544, 464)),
    ("480 x 480: the full height", (80, 0, 560, 480)),
    ("the full frame 640 x 480", (0, 0, 640, 480)),
    ("1 x 1 at (0, 0)", (0, 0, 1, 1)),
    ("1 x 1 at (639, 479)", (639, 479, 640, 480)),
    ("448 x 448 off-centre", (190, 30, 638, 478)),
    ("30 x 460: tall", (500, 10, 530, 470)),
    ("630 x 30: wide", (5, 440, 635, 470)),
    ("301 x 226", (17, 33, 318, 259)),
    ("225 x 223: one pixel off the square", (301, 111, 526, 334)),
    ("2 x 1", (320, 240, 322, 241)),
]


def box_class_renders(seed=611):
    """(names, renders u8 (13,480,640,4), boxes int64 (13,4)): one render per class above."""
    boxes = np.asarray([b for _, b in BOX_CLASSES_480x640], np.int64)
    return [n for n, _ in BOX_CLASSES_480x640], renders_with_boxes(seed, 480, 640, boxes), boxes


# tests/golden/onboard_templates.npz: eight renders at 96 x 128 (tools/make_onboard_golden.py)
GOLDEN_SEED = 601
GOLDEN_SHAPE = (96, 128)
GOLDEN_BOXES = [(36, 20, 92, 76),      # 56 x 56: scale 4, no padding
                (0, 0, 128, 96),       # the full frame
                (127, 95, 128, 96),    # 1 x 1 in the last corner
                (60, 40, 62, 41),      # 2 x 1
                (8, 30, 120, 86),      # 112 x 56: scale 2, the >> 1 shortcut along x, padded rows
                (100, 3, 110, 93),     # 10 x 90: tall
                (11, 7, 48, 30),       # 37 x 23: odd sizes
                (3, 5, 116, 91)]       # 113 x 86


def golden_renders(seed=GOLDEN_SEED):
    H, W = GOLDEN_SHAPE
    return renders_with_boxes(seed, H, W, GOLDEN_BOXES)


def object_renders(seed, N, H, W):
    """N renders of one object: boxes of random position and size, at least 8 pixels a side."""
    rs = np.random.RandomState(seed)
    boxes = []
    for _ in range(N):
        w, h = rs.randint(8, W // 2 + 1), rs.randint(8, H // 2 + 1)
        x0, y0 = rs.randint(0, W - w + 1), rs.randint(0, H - h + 1)
        boxes.append((x0, y0, x0 + w, y0 + h))
    return renders_with_boxes(seed + 1, H, W, boxes)


def object_poses(seed, N):
    return syn.template_geometry(seed, 1, N)[2][0]


def prepare_numpy(rgba, boxes=None, target=224, mean=crop_numpy.CLIP_MEAN, std=crop_numpy.CLIP_STD):
    """TemplateSet.__getitem__ (src/dataloader/template.py:64-70) on the host, by oracle/crop_numpy.py: rgba u8 (N,H,W,4) ->
    (rgb (N,3,T,T), mask (N,T,T), M (N,3,3), boxes).  rgba / 255 is the reference's float64 division rounded to float32
    (template_dataset.py:103)."""
    rgba = np.asarray(rgba)
    if boxes is None:
        boxes = alpha_boxes_numpy(rgba)
    planar = (rgba.transpose(0, 3, 1, 2) / 255).astype(np.float32)
    out, M = crop_numpy.crop_resize_pad(planar, boxes, target)
    rgb = (out[:, :3] - np.asarray(mean, np.float32).reshape(3, 1, 1)) / np.asarray(std, np.float32).reshape(3, 1, 1)
    return rgb.astype(np.float32), np.ascontiguousarray(out[:, 3]), M, np.asarray(boxes, np.int64)


def host_item(rgba, poses, K=syn.TEMPLATE_K, target=224):
    """The item of a template dataset as the host route prepares it: .rgb .mask .K .M .poses as CPU tensors."""
    import torch

    rgb, mask, M, _ = prepare_numpy(rgba, target=target)
    return types.SimpleNamespace(rgb=torch.from_numpy(rgb), mask=torch.from_numpy(mask), K=torch.from_numpy(np.asarray(K, np.float32)),
                                 M=torch.from_numpy(M), poses=torch.from_numpy(np.asarray(poses, np.float32)))
