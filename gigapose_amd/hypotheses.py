"""What the stages behind the matcher share when they draw pose hypotheses: refine.DepthRefiner, verify.HypothesisVerifier and
maskfit.MaskRefiner are HypothesisFlow subclasses and keep only their kernels' calls, their per-chunk state and their read-back;
evaluate.PoseScorer takes its cameras through CameraTable.  No library of its own: host code around render.KeyBuffers.

  pose_matrix(R, t)                                -> (4,4) f64
  projected_boxes(vertices, poses, K, H, W, margin)   the projected model's boxes (host)
  CameraTable(who, cameras, depth, max_pixels)     sorted frames, K, the frame index, H / W, the depth stack and its lazy upload
  check_models(who, models)                        every model has a positive diameter
  grouped(who, estimates, table, models)           estimates by (obj_id, K bytes), groups in order of first appearance
  pack_masks(who, estimates, masks, table)         the two mask forms -> run lengths, offsets, det, areas, boxes (host)
  scan_masks(runs, offsets, H, W, device)          -> (cum, offsets) on the device, what the kernels take as `masks`
  mask_lists(who, masks)                           the check of such a pair
  DeviceMasks(lists, areas, boxes, size)           masks that are on the device already, with what pack_masks works out on the host
  HypothesisFlow                                   the constructor's common part, ._groups(), ._chunks(): the chunk loop
"""
import types

import numpy as np
import torch

from . import _lib, ingest, render

MAX_PAIRS_PER_CALL = 65535                           # the grid's second dimension
MAX_PIXELS = 1 << 22                                 # H*W: the bound on an integer sum


def pose_matrix(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return P


def projected_boxes(vertices, poses, K, H, W, margin):
    """The bounding box of the model's projected vertices at each pose, padded by `margin` pixels: float64 on the host, floor /
    ceil, clamped to [-1, W] x [-1, H] (the kernel clamps to the frame).  A pose that puts a vertex at z <= 0 or gives a value
    that is not finite takes the whole frame.  vertices (V,3), poses (N,4,4), K (N,9) -> int32 (N,4)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    out = np.zeros((len(poses), 4), np.int32)
    for n, (P, k) in enumerate(zip(np.asarray(poses, np.float64), np.asarray(K, np.float64).reshape(-1, 9))):
        p = v @ P[:3, :3].T + P[:3, 3]
        with np.errstate(all="ignore"):
            u = (k[0] * p[:, 0] + k[1] * p[:, 1]) / p[:, 2] + k[2]
            w = (k[4] * p[:, 1]) / p[:, 2] + k[5]
        if not (np.isfinite(u).all() and np.isfinite(w).all() and (p[:, 2] > 0).all()):
            out[n] = (0, 0, W - 1, H - 1)
            continue
        lo = np.clip(np.floor([u.min() - margin, w.min() - margin]), -1, [W, H])
        hi = np.clip(np.ceil([u.max() + margin, w.max() + margin]), -1, [W, H])
        out[n] = (lo[0], lo[1], hi[0], hi[1])
    return out


def join_mask_boxes(box, det, mask_boxes, pad, H, W):
    """box int32 (n,4), IN PLACE: the union with the box of the pair's mask (det >= 0, not empty) padded by `pad` pixels and
    clipped to [-1, W] x [-1, H]."""
    lo, hi = np.clip(mask_boxes[:, :2] - pad, -1, [W, H]), np.clip(mask_boxes[:, 2:] + pad, -1, [W, H])
    d = np.maximum(det, 0)
    use = (det >= 0) & (mask_boxes[d, 2] >= mask_boxes[d, 0])
    box[use, :2], box[use, 2:] = np.minimum(box[use, :2], lo[d[use]]), np.maximum(box[use, 2:], hi[d[use]])


# ------------------------------------------------------------------------------------------------ cameras and models
class CameraTable:
    """cameras {(scene_id, im_id): {"cam_K" 9, ["depth" (H,W)], ["size" (H, W)]}} -> .frames (sorted), .K {frame: f64 (9,)},
    .index {frame: its row of the depth stack}, .H, .W (None until a size is known: .set_size), .depth_host f32 (M,H,W) or None,
    .depth_on(device) its upload, made once.  depth: "required" (every camera has one), "all_or_none", "ignored".  Every
    "depth" and "size" must give the same H x W, of at most max_pixels (None: no limit)."""

    def __init__(self, who, cameras, depth="required", max_pixels=MAX_PIXELS):
        self.max_pixels = max_pixels
        self.frames = sorted(cameras)
        if not self.frames:
            raise ValueError(f"{who}: no cameras")
        self.H = self.W = self.depth_host = self._depth = None
        if depth == "all_or_none":
            with_depth = [k for k in self.frames if cameras[k].get("depth") is not None]
            if with_depth and len(with_depth) != len(self.frames):
                raise ValueError(f"{who}: some cameras have a depth image and some have none (give it for every frame or for none)")
            depth = "required" if with_depth else "ignored"
        if depth == "required":
            maps = [np.asarray(cameras[k]["depth"], np.float32) for k in self.frames]
            self.set_size(who, *maps[0].shape)
            if any(d.shape != (self.H, self.W) for d in maps):
                raise ValueError(f"{who}: the depth images differ in size")
            self.depth_host = np.stack(maps)
        for k in self.frames:
            if cameras[k].get("size") is not None:
                self.set_size(who, *cameras[k]["size"])
        self.K = {k: np.asarray(cameras[k]["cam_K"], np.float64).reshape(9) for k in self.frames}
        self.index = {k: i for i, k in enumerate(self.frames)}

    def set_size(self, who, H, W):
        H, W = int(H), int(W)
        if self.H is not None and (H, W) != (self.H, self.W):
            raise ValueError(f"{who}: frame sizes differ: {H} x {W} and {self.H} x {self.W}")
        if self.max_pixels is not None and (H < 1 or W < 1 or H * W > self.max_pixels):
            raise ValueError(f"{who}: {H} x {W} frames (1 to 2^22 pixels)")
        self.H, self.W = H, W

    def depth_on(self, device):
        if self._depth is None and self.depth_host is not None:
            self._depth = torch.from_numpy(self.depth_host).to(device)
        return self._depth


def check_models(who, models):
    for o, m in models.items():
        if m.get("diameter") is None or not float(m["diameter"]) > 0:
            raise ValueError(f"{who}: model {o} needs a positive diameter")


def grouped(who, estimates, table, models):
    """-> [((obj_id, K bytes), [indices of its estimates, ascending])] in order of first appearance: a group is one mesh under one
    camera matrix, what a draw call takes."""
    groups = {}
    for i, e in enumerate(estimates):
        key, obj = (int(e["scene_id"]), int(e["im_id"])), int(e["obj_id"])
        if key not in table.index:
            raise ValueError(f"{who}: estimate {i}: image {key} has no camera")
        if obj not in models:
            raise ValueError(f"{who}: estimate {i}: object {obj} has no model")
        groups.setdefault((obj, table.K[key].tobytes()), []).append(i)
    return list(groups.items())


def need_gpu(who, device):
    if torch.device(device).type != "cuda":
        raise _lib.GigaPoseHipError(f"{who} needs a GPU device (no CPU fallback)")


# ------------------------------------------------------------------------------------------------ masks
def pack_masks(who, estimates, masks, table):
    """masks: {instance_id: segmentation} or one segmentation per estimate (None = none for it; identical dictionaries are one
    detection), a segmentation a COCO dict {"size": [H, W], "counts": run lengths, or a compressed string (decoded on the host by
    rle_strings)}.  The table learns its frame size from the first mask if it has none.  -> (run lengths int32, offsets int32
    (D+1), det int32 (E,) -1 = none, area f64 (E,) NaN = none, boxes of the masks int64 (D,4) x0 y0 x1 y1 inclusive; W, H, -1, -1
    for an empty mask)."""
    E = len(estimates)
    if isinstance(masks, dict):
        keys, segs = list(masks), list(masks.values())
        index = {k: d for d, k in enumerate(keys)}
        if any("instance_id" not in e for e in estimates):
            raise ValueError(f"{who}: masks keyed by instance_id need estimates with an instance_id (read_hypotheses)")
        det = np.asarray([index.get(int(e["instance_id"]), index.get(e["instance_id"], -1)) for e in estimates], np.int32)
    else:
        masks = list(masks)
        if len(masks) != E:
            raise ValueError(f"{who}: {len(masks)} masks for {E} estimates")
        segs, seen, det = [], {}, np.full(E, -1, np.int32)
        for i, m in enumerate(masks):
            if m is None:
                continue
            if id(m) not in seen:                     # the k hypotheses of a detection usually share one dictionary
                seen[id(m)] = len(segs)
                segs.append(m)
            det[i] = seen[id(m)]
    plain = []
    for d, seg in enumerate(segs):
        if not (isinstance(seg, dict) and "counts" in seg and "size" in seg):
            raise ValueError(f"{who}: mask {d} is not a run-length segmentation {{'size', 'counts'}} (polygons are out of scope)")
        if table.H is None:
            table.set_size(who, *seg["size"])
        if isinstance(seg["counts"], (str, bytes, bytearray)):
            from . import rle_strings

            seg = dict(seg, counts=rle_strings.rle_counts_from_string(seg["counts"]))
        plain.append(seg)
    if table.H is None:
        raise ValueError(f"{who}: the frame size is unknown (no depth image, no camera 'size', no mask)")
    H, W = table.H, table.W
    runs, offsets = ingest.pack_rle(plain, H, W)
    areas, boxes = np.zeros(len(plain)), np.zeros((len(plain), 4), np.int64)
    for d in range(len(plain)):
        c = runs[offsets[d]:offsets[d + 1]].astype(np.int64)
        ones, ends = c[1::2], np.cumsum(c)
        areas[d] = ones.sum()
        first, last = ends[0::2][:len(ones)][ones > 0], (ends[1::2] - 1)[ones > 0]   # the first and last pixel index of each run of ones
        if not len(first):
            boxes[d] = (W, H, -1, -1)
            continue
        wraps = (last // H > first // H).any()                           # a run that passes the end of a column: every row
        boxes[d] = (first.min() // H, 0 if wraps else (first % H).min(), last.max() // H, H - 1 if wraps else (last % H).max())
    area = np.where(det >= 0, areas[np.maximum(det, 0)] if len(plain) else np.nan, np.nan)
    return runs, offsets, det, area, boxes


def scan_masks(runs, offsets, H, W, device):
    """pack_masks' lists -> (cum, offsets) on the device.  pack_rle has checked the lists: the scan's error flag is not read."""
    offsets_d = torch.from_numpy(offsets).to(device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    return ingest.RleDetectionPreprocessor().scan(torch.from_numpy(runs).to(device), offsets_d, H, W, err), offsets_d


class DeviceMasks:
    """Run-length masks that are on the device already (gtinfo.GroundTruthInfo.compute(masks=True) makes them; nothing is packed,
    uploaded or scanned again): .lists = (cum, offsets) as the kernels take them, and what pack_masks works out on the host --
    .areas f64 (D,), .boxes int64 (D,4) x0 y0 x1 y1 inclusive (W, H, -1, -1 for an empty mask; a box may be larger than the mask's
    own: it only has to hold it), .size (H, W).  An estimate names its mask by "instance_id": .index {instance_id: d}, by default
    d itself.  HypothesisVerifier.score takes one as `masks`."""

    def __init__(self, lists, areas, boxes, size, index=None):
        self.lists = mask_lists("DeviceMasks", lists)
        D = self.lists[1].shape[0] - 1
        self.areas, self.boxes = np.asarray(areas, np.float64).reshape(D), np.asarray(boxes, np.int64).reshape(D, 4)
        self.size = (int(size[0]), int(size[1]))
        self.index = {d: d for d in range(D)} if index is None else dict(index)

    def assign(self, who, estimates, table):
        """-> det int32 (E,) -1 = none, area f64 (E,) NaN = none, the masks' boxes: what pack_masks returns after the lists."""
        if any("instance_id" not in e for e in estimates):
            raise ValueError(f"{who}: masks on the device need estimates with an instance_id")
        table.set_size(who, *self.size)
        det = np.asarray([self.index.get(e["instance_id"], -1) for e in estimates], np.int32).reshape(-1)
        area = np.where(det >= 0, self.areas[np.maximum(det, 0)] if len(self.areas) else np.nan, np.nan)
        return det, area, self.boxes


def mask_lists(who, masks, or_none=""):
    """masks = (cum, offsets), int32 (total,) and (D+1,) -> the two, checked."""
    if not (isinstance(masks, (tuple, list)) and len(masks) == 2):
        raise ValueError(f"{who}: masks must be {or_none}(cum, offsets)")
    cum = _lib.arg(masks[0], torch.int32, (None,), who, "cum")
    offsets = _lib.arg(masks[1], torch.int32, (None,), who, "offsets")
    if offsets.shape[0] < 1:
        raise ValueError(f"{who}: offsets holds D + 1 entries, got none")
    return cum, offsets


# ------------------------------------------------------------------------------------------------ the flow
class HypothesisFlow:
    """The part of DepthRefiner, HypothesisVerifier and MaskRefiner that does not depend on what is summed over the drawing:
    .models, .device, .box, .margin, .znear, the camera table (.table; .H, .W, .K, .frames read it), .pairs_per_call, and
      ._groups(who, estimates)   grouped() on the table and the models
      ._chunks(who, estimates, groups, ...)   per group the mesh's upload and one render.KeyBuffers, per chunk of pairs_per_call
                                 estimates what an iteration body needs; nothing synchronises with the host."""

    def __init__(self, who, models, cameras, depth, box, margin, znear, pairs_per_call, device):
        self.models, self.device = models, device
        self.box, self.margin, self.znear = box, float(margin), float(znear)
        self.table = CameraTable(who, cameras, depth)
        self._pairs_per_call = pairs_per_call
        check_models(who, models)

    H, W = property(lambda self: self.table.H), property(lambda self: self.table.W)
    K, frames = property(lambda self: self.table.K), property(lambda self: self.table.frames)

    @property
    def pairs_per_call(self):
        """By default the key buffer of one call stays below render.VIS_BYTES_PER_CALL (the frame size may arrive with the
        first mask)."""
        limit = self._pairs_per_call if self._pairs_per_call is not None else render.VIS_BYTES_PER_CALL // (self.H * self.W * 8)
        return max(1, min(int(limit), MAX_PAIRS_PER_CALL))

    def _groups(self, who, estimates):
        return grouped(who, estimates, self.table, self.models)

    def _chunks(self, who, estimates, groups, boxes=None, det=None, mask_boxes=None, pad=0):
        """boxes int (E,4): the caller's, instead of self.box.  det int32 (E,) with mask_boxes (D,4): each chunk gets its det
        tensor, and a "projected" box is joined with the pair's mask box padded by `pad`.  Yields per chunk a namespace of
          idx      the estimates' indices        first    the chunk opens its group
          model, vertices, faces                 the group's model and its mesh on the device
          poses f64 (nb,4,4), K f64 (nb,9)       on the host
          box int32 (nb,4), frame int32 (nb,) (None without depth), det int32 (nb,) (None without det)   on the device
          draw(poses32, clipped) -> keys (nb,H,W): render.project -> render.raster into the group's buffers"""
        t, dev, step = self.table, self.device, self.pairs_per_call
        H, W = t.H, t.W
        for (obj, _), idx in groups:
            m = self.models[obj]
            vertices, faces = _lib.upload(who, dev, _lib.checked(m["vertices"], torch.float32, (None, 3), who, "vertices"),
                                          _lib.checked(m["faces"], torch.int32, (None, 3), who, "faces"))
            poses_h = np.stack([pose_matrix(estimates[i]["R"], estimates[i]["t"]) for i in idx])
            keys = [(int(estimates[i]["scene_id"]), int(estimates[i]["im_id"])) for i in idx]
            K_h = np.stack([t.K[k] for k in keys])
            if boxes is not None:
                box_h = np.ascontiguousarray(boxes[idx], np.int32)
            elif self.box == "frame":
                box_h = np.tile(np.asarray([0, 0, W - 1, H - 1], np.int32), (len(idx), 1))
            else:
                box_h = projected_boxes(m["vertices"], poses_h, K_h, H, W, self.margin)
                if mask_boxes is not None:
                    join_mask_boxes(box_h, det[idx], mask_boxes, pad, H, W)
            K9 = render._k9(K_h[0])
            buffers = render.KeyBuffers(min(len(idx), step), vertices.shape[0], faces.shape[0], H, W, dev)
            for _, a, b in _lib.chunked(len(idx), step):
                yield types.SimpleNamespace(
                    idx=idx[a:b], first=a == 0, model=m, vertices=vertices, faces=faces, poses=poses_h[a:b], K=np.ascontiguousarray(K_h[a:b]),
                    box=torch.from_numpy(np.ascontiguousarray(box_h[a:b])).to(dev),
                    frame=None if t.depth_host is None else torch.tensor([t.index[k] for k in keys[a:b]], dtype=torch.int32, device=dev),
                    det=None if det is None else torch.from_numpy(np.ascontiguousarray(det[idx[a:b]])).to(dev),
                    draw=lambda poses32, clipped: buffers.draw(vertices, faces, poses32, K9, self.znear, clipped)[0])
