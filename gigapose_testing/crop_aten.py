"""TEST INFRASTRUCTURE ONLY -- the crop stage's reference made from ATen itself, and the box families it is swept over.

`aten_crop_resize_pad` is the documented op sequence of the reference's CropResizePad.__call__ (src/utils/crop.py:16-61)
written with torch ops on CPU tensors: int32 box sizes, `target / max(sizes)` (Tensor.__rtruediv__), Python slicing,
F.interpolate(scale_factor=scale.item()), the pads, F.pad, torch.matmul of the two matrices, F.interpolate(size=(T, T)).
Nothing here restates ATen's arithmetic: whatever index rule, rounding or kernel selection the installed torch has is what
comes out.  oracle/crop_numpy.py (and through it the HIP kernels) is held to this on every family below; the chain itself
is held to the unmodified reference by tests/golden/crop_sizes.npz.

Box families (all seeded, deterministic; boxes are xyxy int64 with a non-negative origin inside the frame -- the reference
would wrap a negative origin Python-style, the project refuses it, so none is generated outside `refused_boxes`):
  long_side_boxes   every long side 1..700 as a square, a wide and a tall box
  doubling_boxes    every (extent, scale) whose first resize doubles the extent or leaves it unchanged under a scale that
                    is not exactly 2 or 1: width only, height only, both -- and extents that put out_h + out_w on either
                    side of ATen's kernel-selection threshold
  identity_boxes    long sides T, 2T, T+-1, 2T+-1, T//2 and T//2+-1
  clamped_boxes     boxes that run past the right / bottom border, with clamped extents in the doubling / identity case
  refused_boxes     boxes for which ATen raises (an empty slice or a scaled side of 0)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

VECTORIZED_MAX_HW = 128      # measured: ATen's CPU upsample_nearest2d takes its shortcut kernel when out_h + out_w <= 128


def index_image(H, W, C=1):
    """pixel = 1 + y*W + x in every channel (+ 0.25 * channel): exact in float32, 0 is left for the padding."""
    base = (1 + np.arange(H * W, dtype=np.float32)).reshape(1, H, W)
    return np.concatenate([base + np.float32(0.25 * c) for c in range(C)], axis=0)


def aten_crop_resize_pad(image, box, target):
    """One item of CropResizePad.__call__: image (C,H,W) float32 CPU tensor, box 4 ints ->
    (images (C,T,T) ndarray, M (3,3) ndarray).  Raises whatever ATen raises."""
    xyxy = torch.as_tensor(np.asarray(box, np.int64)).reshape(1, 4)
    sizes = torch.zeros((1, 2), dtype=torch.int32)                       # BoundingBox.get_box_size
    sizes[:, 0] = xyxy[:, 2] - xyxy[:, 0]
    sizes[:, 1] = xyxy[:, 3] - xyxy[:, 1]
    scale = (target / torch.max(sizes, dim=-1)[0])[0]
    bbox = xyxy[0]
    M_crop = torch.eye(3)
    M_resize_pad = torch.eye(3)
    img = image[:, bbox[1]:bbox[3], bbox[0]:bbox[2]]
    M_crop[:2, 2] = -bbox[:2]
    img = F.interpolate(img.unsqueeze(0), scale_factor=scale.item())[0]
    M_resize_pad[:2, :2] *= scale
    if img.shape[-1] / img.shape[-2] != 1:
        pad_top = (target - img.shape[-2]) // 2
        pad_bottom = max(target - img.shape[-2] - pad_top, 0)
        pad_left = max((target - img.shape[-1]) // 2, 0)
        pad_right = target - img.shape[-1] - pad_left
        img = F.pad(img, [pad_left, pad_right, pad_top, pad_bottom])
        M_resize_pad[:2, 2] = torch.tensor([pad_left, pad_top])
    M = torch.matmul(M_resize_pad, M_crop)
    img = F.interpolate(img.unsqueeze(0), size=(target, target))[0]
    return img.numpy(), M.numpy()


def aten_crop_or_error(image, box, target):
    """(images, M, None) or (None, None, the exception ATen raised)."""
    try:
        img, M = aten_crop_resize_pad(image, box, target)
        return img, M, None
    except (RuntimeError, ValueError, IndexError) as e:
        return None, None, e


def assert_M(M, M_ref, what=""):
    """M[0,0], M[1,1] and the constants bit for bit; the two translations to 1 ulp (the 3-term sums' order is BLAS's)."""
    M, M_ref = np.asarray(M, np.float32).reshape(-1, 3, 3), np.asarray(M_ref, np.float32).reshape(-1, 3, 3)
    exact = np.ones((3, 3), bool)
    exact[:2, 2] = False
    np.testing.assert_array_equal(M[:, exact].view(np.uint32), M_ref[:, exact].view(np.uint32), err_msg=f"M scale/constants {what}")
    np.testing.assert_allclose(M[:, :2, 2], M_ref[:, :2, 2], rtol=2e-7, atol=0, err_msg=f"M translations {what}")


# ---- pure size arithmetic (no torch): what the generators and the class predicates need --------------------------------

def recip_scale(size, target):
    """target / int32_tensor as torch computes it: reciprocal() * target, two float32 roundings."""
    return float((np.float32(1.0) / np.float32(size)) * np.float32(target))


def div_scale(size, target):
    """the correctly rounded float32 quotient -- what the stage computed before it was held to ATen."""
    return float(np.float32(target) / np.float32(size))


def clamped_extent(box, H, W):
    x0, y0, x1, y1 = (int(v) for v in box)
    return min(x1, W) - x0, min(y1, H) - y0


def first_resize(box, H, W, target, scale_of=recip_scale):
    """(cw, ch, w1, h1, scale) of the first resize."""
    x0, y0, x1, y1 = (int(v) for v in box)
    s = scale_of(max(x1 - x0, y1 - y0), target)
    cw, ch = clamped_extent(box, H, W)
    return cw, ch, int(math.floor(cw * s)), int(math.floor(ch * s)), s


def scaled_nonempty(box, H, W, target):
    cw, ch, w1, h1, _ = first_resize(box, H, W, target)
    return cw > 0 and ch > 0 and w1 > 0 and h1 > 0


def is_scale_class(box, H, W, target):
    """Defect class 1: the two-rounding scale and the correctly rounded one give another size after the first resize."""
    a, b = first_resize(box, H, W, target, recip_scale), first_resize(box, H, W, target, div_scale)
    return a[2:4] != b[2:4]


def _shortcut_differs(out, inn, s):
    if out != inn and out != 2 * inn:
        return False
    inv = np.float32(1.0 / s)
    fl = np.minimum(np.floor(np.arange(out, dtype=np.float32) * inv).astype(np.int64), inn - 1)
    return bool((fl != (np.arange(out) >> (1 if out == 2 * inn else 0))).any())


def is_generic_kernel_class(box, H, W, target):
    """Defect class 2, as measured: the first resize runs ATen's generic kernel (out_h + out_w > 128) and has a doubled
    or unchanged dimension whose floored index map is not dst >> 1 / dst."""
    cw, ch, w1, h1, s = first_resize(box, H, W, target)
    if w1 <= 0 or h1 <= 0 or w1 + h1 <= VECTORIZED_MAX_HW:
        return False
    return _shortcut_differs(w1, cw, s) or _shortcut_differs(h1, ch, s)


def is_width_only_doubled(box, H, W, target):
    """The issue's statement of class 2: the first resize doubles the width and not the height."""
    cw, ch, w1, h1, _ = first_resize(box, H, W, target)
    return w1 == 2 * cw and h1 != 2 * ch and h1 > 0


# ---- generators -----------------------------------------------------------------------------------------------------

def _place(rs, w, h, H, W):
    """A box of size w x h with a seeded origin: inside the frame when it fits, else running past the border."""
    x0 = int(rs.randint(0, W - w + 1)) if w <= W else int(rs.randint(0, max(W // 4, 1)))
    y0 = int(rs.randint(0, H - h + 1)) if h <= H else int(rs.randint(0, max(H // 4, 1)))
    return (x0, y0, x0 + w, y0 + h)


def _corner(cw, ch, m, H, W):
    """An m x m box whose clamped extent is cw x ch (needs cw <= min(m, W), ch <= min(m, H))."""
    return (W - cw, H - ch, W - cw + m, H - ch + m)


def long_side_boxes(H, W, target, seed=0, shorts=None, step=1):
    """Every long side 1..700 (every `step`-th), square, wide and tall, the short side from {1, 2, 3, long//2, long-1}
    (or `shorts(long)`).  Boxes whose scaled short side would be 0 belong to `refused_boxes` and are not listed here."""
    rs = np.random.RandomState(seed)
    out = []
    for m in range(1, 701, step):
        out.append(_place(rs, m, m, H, W))
        cand = sorted({c for c in (shorts(m) if shorts else (1, 2, 3, m // 2, m - 1)) if 1 <= c < m})
        for c in cand:
            for b in (_place(rs, m, c, H, W), _place(rs, c, m, H, W)):
                if scaled_nonempty(b, H, W, target):
                    out.append(b)
    return out


def _special_extents(m, target, lim):
    """Extents c <= lim that a box of long side m doubles (floor(c*s) == 2c) or keeps (== c) under a scale != 2, 1."""
    s = recip_scale(m, target)
    if s == 2.0 or s == 1.0 or not (1.0 < s < 3.0):
        return s, []
    k = 2 if s > 2.0 else 1
    return s, [c for c in range(1, min(m, lim) + 1) if int(math.floor(c * s)) == k * c]


def doubling_boxes(H, W, target, seed=0):
    """Every (extent, scale) with floor(extent * s) == 2 * extent (and, the same trap of ATen's shortcut kernel, ==
    extent) at a scale that is not exactly 2 (1): as the width alone, the height alone and both (an m x m box clamped
    in the corner) -- and, for both, partner extents that put out_h + out_w at 128 and 129."""
    rs = np.random.RandomState(seed)
    out = []
    for m in range(1, target + 1):
        s, cs = _special_extents(m, target, max(H, W))
        for c in cs:
            if c < m:
                if c <= W:
                    out.append(_place(rs, c, m, H, W))             # width only (the height is the long side)
                if c <= H:
                    out.append(_place(rs, m, c, H, W))             # height only
            if c <= min(H, W):
                out.append(_corner(c, c, m, H, W))                 # both
            k = int(math.floor(c * s))
            for d in (0, 1):                                       # the other extent chosen for out_h + out_w = 128 + d
                o = int(math.ceil((VECTORIZED_MAX_HW + d - k) / s))
                if (c + d) % 2 == 0 and 1 <= o <= min(m, H) and c <= W:   # the orientation alternates with the extent
                    out.append(_corner(c, o, m, H, W))
                if (c + d) % 2 == 1 and 1 <= o <= min(m, W) and c <= H:
                    out.append(_corner(o, c, m, H, W))
    return out


def identity_boxes(H, W, target, seed=0):
    """Long sides T, 2T, T+-1, 2T+-1, T//2, T//2+-1: first resize the identity / a 2x / one pixel off, final resize live."""
    rs = np.random.RandomState(seed)
    out = []
    for m in (target, 2 * target, target - 1, target + 1, 2 * target - 1, 2 * target + 1, target // 2, target // 2 - 1,
              target // 2 + 1):
        out.append(_place(rs, m, m, H, W))
        for c in sorted({c for c in (1, 2, 3, m // 2, m - 1, m - 2) if 1 <= c < m}):
            for b in (_place(rs, m, c, H, W), _place(rs, c, m, H, W)):
                if scaled_nonempty(b, H, W, target):
                    out.append(b)
    return out


def clamped_boxes(H, W, target, seed=0, n=200):
    """Boxes that run past the right and / or bottom border: seeded random ones, and m x m boxes whose clamped extent is
    exactly doubled, exactly kept (m == T) or one pixel."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        x0, y0 = int(rs.randint(0, W)), int(rs.randint(0, H))
        w, h = int(rs.randint(1, 2 * W)), int(rs.randint(1, 2 * H))
        over = rs.randint(0, 3)                                    # right, bottom, both
        if over != 1:
            w = W - x0 + int(rs.randint(1, W))
        if over != 0:
            h = H - y0 + int(rs.randint(1, H))
        b = (x0, y0, x0 + w, y0 + h)
        if scaled_nonempty(b, H, W, target):
            out.append(b)
    for m in (target, target // 2, 2 * target, target // 2 + 1, target - 1, target // 3, target // 2 - 3):
        for cw, ch in ((1, 1), (1, min(m, H)), (min(m, W), 1), (2, 3), (min(m, W), min(m, H)), (min(m, W) // 2, min(m, H)),
                       (5, min(m, H) // 2)):
            b = _corner(max(cw, 1), max(ch, 1), m, H, W)
            if scaled_nonempty(b, H, W, target):
                out.append(b)
    return out


def refused_boxes(H, W, target):
    """Boxes for which ATen raises: empty or outside the frame (what crop_geometry always refused; the negative origin
    is listed because its Python-style slice is empty as well), and boxes whose scaled short side is 0."""
    out = [(5, 5, 5, 9), (5, 5, 9, 5), (-3, 0, 10, 10), (W + 60, 10, W + 80, 30), (10, H, 20, H + 9), (W, 0, W + 5, 5)]
    for m in (2 * target + 1, 3 * target, 700, 4 * target + 3):
        s = recip_scale(m, target)
        for c in sorted({1, max(int(math.ceil(1.0 / s)) - 1, 1)}):
            if int(math.floor(c * s)) == 0:
                out += [(0, 0, m, c), (1, 2, 1 + c, 2 + m)]
        out.append(_corner(1, 1, m, H, W))                          # clamped to one pixel, scaled to none
    return out


def families(H, W, target, seed=0, thin=False):
    """name -> boxes.  `thin` keeps every third long side with two short sides: for the targets after the first."""
    long_kw = dict(step=3, shorts=lambda m: (2, m // 2)) if thin else {}
    return {
        "long_side": long_side_boxes(H, W, target, seed, **long_kw),
        "doubling": doubling_boxes(H, W, target, seed + 1),
        "identity": identity_boxes(H, W, target, seed + 2),
        "clamped": clamped_boxes(H, W, target, seed + 3),
        "refused": refused_boxes(H, W, target),
    }


# ---- the GPU tests' and the second golden's box list ----------------------------------------------------------------

GPU_FRAME = (97, 131)        # H, W


def gpu_boxes(target):
    """About 64 boxes on a 97x131 frame, taken from the families above: (boxes int64 (n,4), refused int64 (k,4)) at
    `target` -- a narrow box whose short side scales to nothing at a small target moves to the refused ones.  The
    scale-class long sides are the same at 224, 112 and 56: the scale only changes by a power of two between them."""
    H, W = GPU_FRAME
    b = []
    # scale class: long sides whose two-rounding scale moves the scaled long side (non-square: a pad row appears / goes)
    for i, m in enumerate((23, 24, 41, 46, 48, 49, 67, 69, 82, 92, 95, 96)):
        c = (m // 3, m // 2, m - 1, m // 2, m - 1, m // 4)[i % 6]
        b.append((3 + i, 1, 3 + i + m, 1 + c) if i % 2 == 0 else (2 * i, 0, 2 * i + c, m))
    b += [(7, 9, 7 + 121, 9 + 60), (0, 30, 123, 30 + 2), (10, 0, 10 + 47, 95), (9, 1, 76, 2)]
    # generic-kernel class at 224: a doubled (long side <= 111) or kept (112..223) extent next to a long side near 224
    b += [(40, 3, 42, 93), (7, 0, 10, 97), (10, 0, 30, 110), (100, 0, 127, 110), (50, 2, 55, 107)]      # width only doubled
    b += [(5, 50, 95, 52), (0, 10, 110, 30), (11, 60, 121, 87), (20, 90, 125, 95), (0, 0, 100, 4)]      # height only doubled
    b += [(0, 10, 222, 60), (5, 0, 45, 220), (0, 0, 223, 97), (60, 0, 131, 223)]                        # kept extents, 1 < s < 2
    # both doubled, on either side of the kernel threshold out_h + out_w = 128: 111 x 111 boxes clamped in the corner
    b += [_corner(cw, ch, 111, H, W) for cw, ch in ((32, 32), (33, 32), (32, 33), (50, 14), (50, 15), (14, 50), (2, 2))]
    b += [_corner(2, 2, 90, H, W), _corner(20, 11, 100, H, W)]
    # identity and 2x (exact scales), final resize one pixel off, clamped
    b += [(0, 0, 224, 224), (10, 5, 234, 229), (19, 0, 131, 97), (0, 0, 112, 56), (60, 50, 60 + 112, 50 + 112),
          (0, 0, 223, 223), (0, 0, 225, 100), (3, 0, 3 + 113, 97), (20, 0, 131, 97), (0, 0, 37, 37), (4, 4, 41, 30),
          (0, 0, 74, 74), (9, 9, 9 + 75, 9 + 18), (1, 0, 1 + 36, 97), (0, 0, 131, 97), (0, 0, 448, 448), (0, 0, 449, 97)]
    b += [(100, 60, 190, 150), (W - 1, H - 1, W + 50, H + 20), (W - 7, 3, W + 4, 30), (5, H - 3, 60, H + 33),
          (120, 90, 143, 113), (0, 96, 131, 120)]
    b += [(64, 48, 65, 49), (64, 48, 66, 49), (0, 0, 7, 3)]                                               # tiny
    refused = [(5, 5, 5, 9), (W + 3, 10, W + 30, 30), (0, 0, 700, 1), (W - 1, H - 1, W - 1 + 500, H - 1 + 500)]
    live = [x for x in b if scaled_nonempty(x, H, W, target)]
    refused += [x for x in b if not scaled_nonempty(x, H, W, target)]
    return np.asarray(live, np.int64), np.asarray(refused, np.int64)


def aten_batch(images, boxes, target):
    """aten_crop_resize_pad per item: images (D,C,H,W) or one shared (C,H,W) ndarray -> (images (D,C,T,T), M (D,3,3))."""
    t = torch.from_numpy(np.ascontiguousarray(images))
    outs = [aten_crop_resize_pad(t if t.dim() == 3 else t[d], box, target) for d, box in enumerate(boxes)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def aten_preprocess_detections(rgb_u8, masks, boxes, im_id, target, mean, std):
    """process_real + normalize around the ATen chain: rgb / 255 * mask, the RGBA stack cropped by ATen, (x - mean) / std --
    the pointwise float32 steps as oracle/crop_numpy.preprocess_detections has them.  -> tar_img, tar_mask, M."""
    rgb = rgb_u8.astype(np.float32) / np.float32(255.0)
    rgba = np.concatenate([rgb[im_id] * masks[:, None], masks[:, None]], axis=1)
    out, M = aten_batch(rgba, boxes, target)
    mean, std = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
    return ((out[:, :3] - mean) / std).astype(np.float32), out[:, 3], M


def gpu_case(target, seed=77):
    """The GPU tests' inputs at `target`: one 97x131 u8 frame, a ragged binary mask per live box (about 3 pixels in 4
    set), the live and the refused boxes."""
    H, W = GPU_FRAME
    boxes, refused = gpu_boxes(target)
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, (1, 3, H, W)).astype(np.uint8)
    masks = (rs.rand(len(boxes), H, W) < 0.75).astype(np.float32)
    return dict(rgb=rgb, masks=masks, boxes=boxes, refused=refused, im_id=np.zeros(len(boxes), np.int32))
