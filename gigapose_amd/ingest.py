"""Frames in: a u8 camera frame plus CNOS detections (xywh box, category, score, run-length mask) -> the batch GigaPose.test_step
consumes, with the masks decoded ON the GPU while the crops are taken (libgigapose_ingest.so, C-ABI: include/gigapose_ingest.h).

The reference builds that batch on the CPU (GigaPoseTestSet.add_detections / collate_fn, src/dataloader/test.py:205-318, with
process_real, src/dataloader/train.py:80-123): every mask is expanded from its run-length list to a dense H x W array by a Python
loop, stacked as a float RGBA tensor per detection, cropped one by one and normalised.  `crop.DetectionPreprocessor` moved the
crop to the GPU but takes dense f32 masks (1.2 MB per detection at 480 x 640); here a frame (0.92 MB) and its run lists (a few
KB) are all that crosses PCIe.

Mask format -- uncompressed COCO run-length encoding, exactly what src/utils/mask.py:mask_to_rle writes:
  - `size = [H, W]`;
  - `counts` holds the lengths of alternating runs of 0 and 1 over the mask flattened COLUMN-major: pixel (y, x) has index
    p = x*H + y;
  - the first run is zeros and may have length 0;
  - the counts sum to H*W;
  - with cum the inclusive prefix sums, pixel p lies in run j = #{i : cum[i] <= p}, and its value is j & 1.
Compressed string `counts` (pycocotools' byte coding) are out of scope: `pack_rle` raises a ValueError that says so.

  mask_to_rle_counts(mask)            the format as a vectorised numpy encoder
  pack_rle(segmentations, H, W)       list of {"counts", "size"} -> (counts int32[total], offsets int32[D+1]), checked
  RleDetectionPreprocessor            DetectionPreprocessor with (counts, offsets) in place of the dense masks; same results, bit for bit
  FrameIngest                         frames + CNOS dicts -> PandasTensorCollection (tar_img, tar_mask, tar_K, tar_M, infos, .test_list)
There is no CPU fallback: the kernels need the GPU, a missing library is an error.
"""
import ctypes

import numpy as np
import pandas as pd
import torch

from . import _lib
from .crop import CLIP_MEAN, CLIP_STD
from .tensor_collection import PandasTensorCollection

_ingest = _lib.SideLibrary("libgigapose_ingest.so", "gpi")
INGEST_LIB_PATH, lib, _call = _ingest.path, _ingest.lib, _ingest.call


# ------------------------------------------------------------------------------------------------ host side: the format
def mask_to_rle_counts(mask):
    """(H,W) array, non-zero = set -> int32 run lengths, equal to mask_to_rle(mask)["counts"] (src/utils/mask.py:9-27) for a
    binary mask, without its per-pixel Python loop."""
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError(f"mask_to_rle_counts: expected an (H, W) mask, got shape {mask.shape}")
    flat = mask.ravel(order="F") != 0
    if flat.size == 0:
        return np.zeros(1, np.int32)
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate(([0], edges, [flat.size])))
    if flat[0]:                                       # the first run is zeros: empty when pixel (0, 0) is set
        counts = np.concatenate(([0], counts))
    return counts.astype(np.int32)


def pack_rle(segmentations, H, W):
    """List of {"counts": [...], "size": [H, W]} (the `segmentation` of a CNOS detection) -> (counts int32[total], offsets
    int32[D+1]): detection d owns counts[offsets[d]:offsets[d+1]].  Raises ValueError, naming the detection, on a size other than
    [H, W], string (compressed) counts, a negative count or counts that do not sum to H*W."""
    H, W = int(H), int(W)
    if not (H > 0 and W > 0 and H * W < 2 ** 31):
        raise ValueError(f"pack_rle: frame size {H} x {W} is not supported (0 < H*W < 2^31)")
    lists, offsets = [], [0]
    for d, seg in enumerate(segmentations):
        size, counts = list(seg["size"]), seg["counts"]
        if [int(s) for s in size] != [H, W]:
            raise ValueError(f"pack_rle: detection {d}: mask size {size} does not match the frame size [{H}, {W}]")
        if isinstance(counts, (str, bytes)):
            raise ValueError(f"pack_rle: detection {d}: compressed string counts (pycocotools' byte coding) are out of scope; "
                             "pass uncompressed integer run lengths")
        c = np.asarray(counts, dtype=np.int64).reshape(-1)
        if (c < 0).any():
            raise ValueError(f"pack_rle: detection {d}: negative run length {int(c[c < 0][0])}")
        if int(c.sum()) != H * W:
            raise ValueError(f"pack_rle: detection {d}: the run lengths sum to {int(c.sum())}, not H*W = {H * W}")
        lists.append(c.astype(np.int32))
        offsets.append(offsets[-1] + len(c))
    if offsets[-1] >= 2 ** 30:
        raise ValueError(f"pack_rle: {offsets[-1]} runs in one batch (the limit is 2^30)")
    counts = np.concatenate(lists) if lists else np.zeros(0, np.int32)
    return counts.astype(np.int32), np.asarray(offsets, np.int32)


def xywh_to_xyxy_long(bboxes):
    """BoundingBox(bboxes, "xywh").xyxy_box (src/utils/bbox.py:5-21, 116-131): [x, y, x+w, y+h] in the input's float type -- a
    list becomes float32, the `.float()` of megapose/datasets/scene_dataset.py:337 -- then truncated toward zero as `.long()` does."""
    b = np.asarray(bboxes)
    if isinstance(bboxes, (list, tuple)) or not np.issubdtype(b.dtype, np.floating):
        b = b.astype(np.float32)
    b = b.reshape(-1, 4)
    xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1)
    return np.trunc(xyxy).astype(np.int64)


def host_batch(infos, detections, H, W, label_map=None):
    """The host half of FrameIngest: per-image CNOS detection lists -> (counts, offsets, xyxy int64 (D,4), im_id int32 (D),
    infos DataFrame with one row per detection, in detection order).  add_detections (src/dataloader/test.py:205-242): label =
    str(category_id), the score stands in for visib_fract; `label_map` is the caller's renumbering (LM-O: test.py:302-306)."""
    if len(infos) != len(detections):
        raise ValueError(f"FrameIngest: {len(infos)} image infos for {len(detections)} detection lists")
    segs, boxes, rows = [], [], []
    for im, (info, dets) in enumerate(zip(infos, detections)):
        scene_id, view_id = int(_field(info, "scene_id")), int(_field(info, "view_id"))
        for det in dets:
            label = int(det["category_id"])
            if label_map is not None:
                label = label_map[label]
            segs.append(det["segmentation"])
            boxes.append(det["bbox"])
            rows.append(dict(label=str(label), scene_id=scene_id, view_id=view_id, batch_im_id=im, visib_fract=float(det["score"])))
    counts, offsets = pack_rle(segs, H, W)
    xyxy = xywh_to_xyxy_long(np.asarray(boxes, np.float32).reshape(-1, 4))
    im_id = np.asarray([r["batch_im_id"] for r in rows], np.int32)
    frame = pd.DataFrame(rows, columns=["label", "scene_id", "view_id", "batch_im_id", "visib_fract"])
    return counts, offsets, xyxy, im_id, frame


def _field(info, name):
    return info[name] if isinstance(info, dict) or hasattr(info, "keys") else getattr(info, name)


# ------------------------------------------------------------------------------------------------ device side
class RleDetectionPreprocessor:
    """frames uint8 (n_img,3,H,W) + per-detection run lists / boxes / frame ids -> what DetectionPreprocessor returns for the
    dense masks the lists encode: {"tar_img", "tar_mask", "tar_M"}, bit for bit."""

    def __init__(self, target_size=224, mean=CLIP_MEAN, std=CLIP_STD):
        self.target_size = target_size
        self._mean = (ctypes.c_float * 3)(*mean)
        self._std = (ctypes.c_float * 3)(*std)

    @staticmethod
    def _dev(a, dev, dtype):
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        return t.to(device=dev, dtype=dtype).contiguous()

    @torch.no_grad()
    def scan(self, counts, offsets, H, W, err):
        """counts int32[total], offsets int32[D+1] on the device -> cum int32[total] (gpi_rle_scan)."""
        cum = torch.empty_like(counts)
        _call("gpi_rle_scan", counts, offsets, counts.numel(), offsets.numel() - 1, H, W, cum, err, _lib.stream_ptr())
        return cum

    def _inputs(self, counts, offsets, dev):
        """What the scan reads, on the device; the last two are (counts, offsets)."""
        counts, offsets = self._dev(counts, dev, torch.int32), self._dev(offsets, dev, torch.int32)
        assert counts.dim() == 1 and offsets.dim() == 1
        return counts, offsets

    def _scan(self, lists, H, W, err):
        """The step a subclass replaces: what _inputs returned -> cum."""
        return self.scan(*lists, H, W, err)

    @torch.no_grad()
    def decode(self, counts, offsets, H, W):
        """The dense masks (D,H,W) f32 the lists encode (gpi_rle_decode): the reference's scene_obs.binary_masks."""
        return self._decode((counts, offsets), counts.device, H, W)

    def _decode(self, lists, dev, H, W):
        lists = self._inputs(*lists, dev)
        counts, offsets = lists[-2:]
        D = offsets.numel() - 1
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        cum = self._scan(lists, H, W, err)
        masks = torch.zeros(D, H, W, device=dev)
        _call("gpi_rle_decode", cum, offsets, counts.numel(), D, H, W, masks, _lib.stream_ptr())
        bad = int(err.item())
        if bad:
            raise ValueError(f"{type(self).__name__}.decode: detection {bad - 1} has a bad run-length list (no run, a negative "
                             f"run or a total other than H*W = {H * W})")
        return masks

    @torch.no_grad()
    def __call__(self, rgb_u8, counts, offsets, xyxy_boxes, batch_im_id):
        return self._crop(rgb_u8, (counts, offsets), xyxy_boxes, batch_im_id)

    def _crop(self, rgb_u8, lists, xyxy_boxes, batch_im_id, **how):
        who = type(self).__name__
        if not (isinstance(rgb_u8, torch.Tensor) and rgb_u8.is_cuda):
            raise _lib.GigaPoseHipError(f"{who} needs the frames on the GPU (no CPU fallback)")
        dev = rgb_u8.device
        assert rgb_u8.dtype == torch.uint8 and rgb_u8.dim() == 4 and rgb_u8.shape[1] == 3
        rgb_u8 = rgb_u8.contiguous()
        lists = self._inputs(*lists, dev, **how)
        counts, offsets = lists[-2:]
        boxes = self._dev(xyxy_boxes, dev, torch.int64)
        im_id = self._dev(batch_im_id, dev, torch.int32)
        n_img, _, H, W = rgb_u8.shape
        D, T = offsets.numel() - 1, self.target_size
        assert D >= 0 and boxes.shape == (D, 4) and im_id.shape == (D,)
        tar_img = torch.empty(D, 3, T, T, device=dev)
        tar_mask = torch.empty(D, T, T, device=dev)
        M = torch.empty(D, 3, 3, device=dev)
        if D == 0:
            return {"tar_img": tar_img, "tar_mask": tar_mask, "tar_M": M}
        err = torch.zeros(2, dtype=torch.int32, device=dev)     # [0]: the scan's flag, [1]: the crop's
        cum = self._scan(lists, H, W, err[0:1])
        _call("gpi_preprocess_detections_rle", rgb_u8, cum, offsets, counts.numel(), boxes, im_id, n_img, D, H, W, T, self._mean, self._std, tar_img, tar_mask,
              M, err[1:2], _lib.stream_ptr())
        bad_list, bad_box = err.tolist()  # one host sync per batch, where DetectionPreprocessor has its own
        if bad_list:
            raise ValueError(f"{who}: detection {bad_list - 1} has a bad run-length list (no run, a negative run "
                             f"or a total other than H*W = {H * W})")
        if bad_box:
            raise ValueError(f"{who}: detection {bad_box - 1} has an empty / out-of-frame box")
        return {"tar_img": tar_img, "tar_mask": tar_mask, "tar_M": M}


def lay_pinned(parts):
    """(name, array) parts laid end to end into ONE pinned u8 buffer -> (buffer, {name: (first byte, past the last, shape)})."""
    spans, at = {}, 0
    for name, a in parts:
        spans[name] = (at, at + a.nbytes, a.shape)
        at += a.nbytes
    buf = torch.empty(max(at, 1), dtype=torch.uint8, pin_memory=True)
    view = buf.numpy()
    for name, a in parts:
        view[spans[name][0]:spans[name][1]] = a.reshape(-1).view(np.uint8)
    return buf, spans


class FrameIngest:
    """Detector output + camera frames -> the batch of GigaPoseTestSet.collate_fn's no-ground-truth branch
    (src/dataloader/test.py:301-315): PandasTensorCollection(tar_img, tar_mask, tar_K, tar_M, infos) with the attribute test_list.

    Host to device: counts, offsets, boxes, image ids (and the 3x3 intrinsics) travel in ONE pinned staging buffer with one
    non-blocking copy on the current stream; the frames are a second copy (non-blocking when they sit in pinned memory).  The only
    host synchronisation is the error-flag read of RleDetectionPreprocessor."""

    def __init__(self, target_size=224, mean=CLIP_MEAN, std=CLIP_STD, device="cuda"):
        self.target_size = target_size
        self.device = torch.device(device)
        self.preprocess = RleDetectionPreprocessor(target_size, mean, std)

    @staticmethod
    def stage(counts, offsets, xyxy, im_id, K):
        """The pinned staging buffer: [boxes i64 | counts i32 | offsets i32 | im_id i32 | K f32] and the byte spans of its parts."""
        return lay_pinned([("boxes", np.ascontiguousarray(xyxy, np.int64)), ("counts", np.ascontiguousarray(counts, np.int32)),
                           ("offsets", np.ascontiguousarray(offsets, np.int32)), ("im_id", np.ascontiguousarray(im_id, np.int32)),
                           ("K", np.ascontiguousarray(K, np.float32))])

    @staticmethod
    def _frames(frames_u8, K, detections):
        """The frame / K checks -> (frames tensor, K as numpy, H, W)."""
        if isinstance(frames_u8, np.ndarray):
            frames_u8 = torch.from_numpy(frames_u8)
        assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[1] == 3
        n_img, _, H, W = frames_u8.shape
        K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
        assert K.shape == (n_img, 3, 3) and len(detections) == n_img
        return frames_u8, K, H, W

    @staticmethod
    def _batch(frame, test_list, **tensors):
        batch = PandasTensorCollection(infos=frame, **tensors)
        batch.test_list = test_list
        return batch

    def _empty(self, frame, test_list):
        dev, T = self.device, self.target_size
        return self._batch(frame, test_list, tar_img=torch.empty(0, 3, T, T, device=dev), tar_mask=torch.empty(0, T, T, device=dev),
                           tar_K=torch.empty(0, 3, 3, device=dev), tar_M=torch.empty(0, 3, 3, device=dev))

    def _preprocess(self, frames, part, boxes, im):
        return self.preprocess(frames, part("counts", torch.int32), part("offsets", torch.int32), boxes, im)

    def _finish(self, dbuf, spans, frame, frames, test_list):
        """The staged buffer on the device -> the batch."""
        def part(name, dtype):
            a, b, shape = spans[name]
            return dbuf[a:b].view(dtype).view(shape)

        im = part("im_id", torch.int32)
        out = self._preprocess(frames, part, part("boxes", torch.int64), im)
        tar_K = part("K", torch.float32).index_select(0, im.long())        # data.K[idx_selected].float() (train.py:102)
        return self._batch(frame, test_list, tar_img=out["tar_img"], tar_mask=out["tar_mask"], tar_K=tar_K, tar_M=out["tar_M"])

    @torch.no_grad()
    def __call__(self, frames_u8, K, infos, detections, test_list=None, label_map=None):
        """frames_u8 (n_img,3,H,W) u8 (host, ideally pinned, or already on the device), K (n_img,3,3), infos: per image scene_id
        and view_id, detections: per image the list of CNOS dicts (bbox xywh, category_id, score, segmentation, optional time)."""
        frames_u8, K, H, W = self._frames(frames_u8, K, detections)
        counts, offsets, xyxy, im_id, frame = host_batch(infos, detections, H, W, label_map)
        if len(im_id) == 0:
            return self._empty(frame, test_list)
        buf, spans = self.stage(counts, offsets, xyxy, im_id, K)
        dbuf = buf.to(self.device, non_blocking=True)
        return self._finish(dbuf, spans, frame, frames_u8.to(self.device, non_blocking=True), test_list)
