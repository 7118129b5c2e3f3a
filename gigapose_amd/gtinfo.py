"""What scene_gt_info.json and the mask / mask_visib images of a BOP dataset hold, computed ON the GPU for ground truths drawn by
the compute rasteriser (libgigapose_gtinfo.so, C-ABI: include/gigapose_gtinfo.h, which spells the rules out;
gigapose_testing/gtinfo_ref.py restates them in numpy and tests/test_gpu_gtinfo.py holds the kernels to it bit for bit).
bop_toolkit makes these files with an OpenGL renderer (scripts/calc_gt_info.py, calc_gt_masks.py); an Instinct accelerator has
none.  BOP-19 recall is defined over the ground truths that are at least 10 % visible: `visib_fract` is what
evaluate.PoseScorer(min_visib=0.1) and distances.AddScorer(min_visib=0.1) read, and the visible masks are what the
mask-consuming stages (verify, maskfit) take as `masks`.

  classify(vis, origin, depth, frame, ray, ray_index, delta)   -> cls u8 (N,W,H), info int64 (N,4), box int32 (N,8), status int32 (N,)
  encode_runs(cls, which)                      -> (counts, cum, offsets): the uncompressed COCO run lengths of every instance
  GroundTruthInfo(models, cameras, ...)        .compute(gts, masks=False) -> {(scene_id, im_id): [per instance a dict]}
  with_visibility(gts, info)                   gts whose entries carry "visib_fract"
Out of scope: the bop18 visibility mode, reading or writing the json / PNG files, polygon masks, compressed COCO strings on
output (only uncompressed `counts`), near-plane clipping (a ground truth that drops a triangle raises).  There is no CPU
fallback: a missing library is an error.
"""
import math

import numpy as np
import torch

from . import _lib, render
from .evaluate import ray_map
from .hypotheses import MAX_PAIRS_PER_CALL, MAX_PIXELS, CameraTable, DeviceMasks, grouped, need_gpu, pose_matrix

INFO, BOX = 4, 8
PX_ALL, PX_FRAME, PX_VALID, PX_VISIB = 0, 1, 2, 3
BOX_EMPTY_MIN, BOX_EMPTY_MAX = 2 ** 30, -2 ** 30
CLS_OBJECT, CLS_VISIBLE = 1, 2
BAD_FRAME, BAD_RAY = 1, 2
STATUS_BITS = {BAD_FRAME: "the frame index lies outside the depth stack", BAD_RAY: "the ray index lies outside the ray maps"}
MAX_CANVAS_PIXELS = 2 ** 31 - 1                      # Hc*Wc < 2^31 (gigapose_gtinfo.h: Limits)
_gtinfo = _lib.SideLibrary("libgigapose_gtinfo.so", "gpg")
GTINFO_LIB_PATH, lib, _call = _gtinfo.path, _gtinfo.lib, _gtinfo.call


def pixels_per_workgroup():
    return int(lib().gpg_pixels_per_workgroup())


def runs_workspace_bytes(N, H, W):
    return _gtinfo.value("gpg_runs_workspace_bytes", N, H, W)


@torch.no_grad()
def classify(vis, origin, depth, frame, ray, ray_index, delta):
    """gpg_classify: vis int64 (N,Hc,Wc) holding render.raster's keys on the canvas; origin = (ox, oy): frame pixel (x, y) is
    canvas pixel (x + ox, y + oy); depth f32 (M,H,W) or None (then frame is not read and may be None); frame int32 (N,); ray
    f64 (R,H,W), the ray map of the FRAME (evaluate.ray_map), which gives H and W; ray_index int32 (N,); all on the device
    -> cls u8 (N,W,H) column-major (bit 0 object, bit 1 visible), info int64 (N,4) = px_count_all, object pixels in the frame,
    px_count_valid, px_count_visib; box int32 (N,8) = min x, min y, max x, max y of the object (over the canvas, in frame
    coordinates) and of the visible pixels, 2^30, 2^30, -2^30, -2^30 where empty; status int32 (N,).  N <= 65535, H*W <= 2^22,
    Hc*Wc < 2^31."""
    who = "classify"
    vis = _lib.arg(vis, torch.int64, (None, None, None), who, "vis")
    N, Hc, Wc = vis.shape
    ray = _lib.arg(ray, torch.float64, (None, None, None), who, "ray")
    R, H, W = ray.shape
    given = dict(vis=vis, ray=ray)
    if depth is not None:
        given["depth"] = depth = _lib.arg(depth, torch.float32, (None, H, W), who, "depth")
        given["frame"] = frame = _lib.arg(frame, torch.int32, (N,), who, "frame")
    else:
        frame = None
    given["ray_index"] = ray_index = _lib.arg(ray_index, torch.int32, (N,), who, "ray_index")
    ox, oy = (int(v) for v in origin)
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} instances in one call (at most {MAX_PAIRS_PER_CALL}: GroundTruthInfo chunks)")
    if H < 1 or W < 1 or H * W > MAX_PIXELS or R < 1 or (depth is not None and depth.shape[0] < 1):
        raise ValueError(f"{who}: bad sizes (H, W > 0, H*W <= 2^22, M, R >= 1)")
    if Hc < 1 or Wc < 1 or Hc * Wc > MAX_CANVAS_PIXELS or max(Hc, Wc) > 2 ** 30:
        raise ValueError(f"{who}: bad canvas {Hc} x {Wc} (Hc*Wc < 2^31)")
    if not (0 <= ox and ox + W <= Wc and 0 <= oy and oy + H <= Hc):
        raise ValueError(f"{who}: the {H} x {W} frame at origin ({ox}, {oy}) leaves the {Hc} x {Wc} canvas")
    if math.isnan(delta):
        raise ValueError(f"{who}: delta is NaN")
    _lib.on_gpu(who, **given)
    dev = vis.device
    cls = torch.empty(N, W, H, dtype=torch.uint8, device=dev)
    info = torch.empty(N, INFO, dtype=torch.int64, device=dev)
    box = torch.empty(N, BOX, dtype=torch.int32, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    _call("gpg_classify", vis, Hc, Wc, ox, oy, depth, 0 if depth is None else depth.shape[0], frame, ray, R, ray_index, delta, N, H, W, cls, info, box, status,
          _lib.stream_ptr())
    return cls, info, box, status


def _cls_arg(who, cls, which):
    cls = _lib.arg(cls, torch.uint8, (None, None, None), who, "cls")
    N, W, H = cls.shape
    if which not in (0, 1):
        raise ValueError(f"{who}: which must be 0 (the object bit) or 1 (the visible bit), got {which!r}")
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"{who}: bad sizes (H, W > 0, H*W <= 2^22)")
    return cls, N, H, W


@torch.no_grad()
def count_runs(cls, which, workspace=None):
    """gpg_count_runs: cls u8 (N,W,H) on the device, N <= 65535 -> runs int32 (N,), the workspace (int64) gpg_write_runs reads."""
    who = "count_runs"
    cls, N, H, W = _cls_arg(who, cls, which)
    if N > MAX_PAIRS_PER_CALL:
        raise ValueError(f"{who}: {N} instances in one call (at most {MAX_PAIRS_PER_CALL}: encode_runs chunks)")
    _lib.on_gpu(who, cls=cls)
    need = max(1, runs_workspace_bytes(N, H, W) // 8)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.int64, device=cls.device)
    workspace = _lib.arg(workspace, torch.int64, (None,), who, "workspace")
    if workspace.numel() < need:
        raise ValueError(f"{who}: the workspace is too small ({workspace.numel() * 8} < {need * 8} bytes)")
    _lib.on_gpu(who, workspace=workspace)
    runs = torch.empty(N, dtype=torch.int32, device=cls.device)
    _call("gpg_count_runs", cls, N, H, W, which, runs, workspace, _lib.stream_ptr())
    return runs, workspace


@torch.no_grad()
def write_runs(cls, which, workspace, offsets, out, err):
    """gpg_write_runs: the cls, which and workspace of count_runs; offsets int32 (N+1,); out = (counts, cum), int32 (total,) each,
    written in place; err int32 (1,): zeroed by the call, n + 1 of an instance whose slice does not fit afterwards."""
    who = "write_runs"
    cls, N, H, W = _cls_arg(who, cls, which)
    workspace = _lib.arg(workspace, torch.int64, (None,), who, "workspace")
    offsets = _lib.arg(offsets, torch.int32, (N + 1,), who, "offsets")
    counts = _lib.arg(out[0], torch.int32, (None,), who, "counts")
    cum = _lib.arg(out[1], torch.int32, (counts.shape[0],), who, "cum")
    err = _lib.arg(err, torch.int32, (1,), who, "err")
    if N > MAX_PAIRS_PER_CALL or workspace.numel() * 8 < runs_workspace_bytes(N, H, W):
        raise ValueError(f"{who}: more than {MAX_PAIRS_PER_CALL} instances, or the workspace is not count_runs'")
    _lib.on_gpu(who, cls=cls, workspace=workspace, offsets=offsets, counts=counts, cum=cum, err=err)
    _call("gpg_write_runs", cls, N, H, W, which, workspace, offsets, counts.shape[0], counts, cum, err, _lib.stream_ptr())
    return counts, cum


@torch.no_grad()
def encode_runs(cls, which):
    """cls u8 (N,W,H) on the device (any N: chunked at 65535), which = 0: the object bit, 1: the visible bit
    -> (counts int32 (total,), cum int32 (total,), offsets int32 (N+1,)) on the device: instance n owns [offsets[n], offsets[n+1]),
    counts are COCO's uncompressed run lengths over the mask flattened column-major (the first run is zeros), cum their inclusive
    prefix sums -- bit for bit what ingest's scan leaves for counts, so (cum, offsets) is what verify.counts and maskfit take as
    `masks`.  ONE host synchronisation, between the two kernels: the lists are sized from the run counts."""
    who = "encode_runs"
    cls, N, H, W = _cls_arg(who, cls, which)
    _lib.on_gpu(who, cls=cls)
    dev = cls.device
    parts = [(a, b) + count_runs(cls[a:b], which) for _, a, b in _lib.chunked(N, MAX_PAIRS_PER_CALL)]
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if N:
        offsets[1:] = torch.cumsum(torch.cat([p[2] for p in parts]), 0)
    total = int(offsets[-1])                                     # the synchronisation
    if total >= 2 ** 31:
        raise ValueError(f"{who}: {total} runs in one batch (the lists are indexed with 32 bits: encode fewer instances per call)")
    offsets = offsets.to(torch.int32)
    counts, cum = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for a, b, _, work in parts:
        write_runs(cls[a:b], which, work, offsets[a:b + 1], (counts, cum), err)
    return counts, cum, offsets


# ------------------------------------------------------------------------------------------------ the ground truths of a dataset
def canvas(H, W, margin):
    """-> Hc, Wc, ox, oy: `margin` frame sizes on every side, rounded up to whole pixels."""
    ox, oy = int(math.ceil(margin * W)), int(math.ceil(margin * H))
    return H + 2 * oy, W + 2 * ox, ox, oy


def largest_margin(H, W):
    """The largest margin, to 1/1000 and rounded down, whose canvas has Hc*Wc < 2^31 (the canvas grows with the margin)."""
    lo, hi = 0, 1000 * (MAX_CANVAS_PIXELS // min(H, W) + 1)      # in thousandths: lo fits (the frame itself does), hi does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        Hc, Wc, _, _ = canvas(H, W, mid / 1000.0)
        lo, hi = (mid, hi) if Hc * Wc <= MAX_CANVAS_PIXELS else (lo, mid)
    return lo / 1000.0


def box_xywh(corners):
    """min x, min y, max x, max y -> [x, y, w, h], or [-1, -1, -1, -1] for the initial values of an empty set."""
    x0, y0, x1, y1 = (int(v) for v in corners)
    return [-1, -1, -1, -1] if x1 < x0 else [x0, y0, x1 - x0 + 1, y1 - y0 + 1]


class GroundTruthTable(dict):
    """What GroundTruthInfo.compute returns: {(scene_id, im_id): [per instance a dict]}, and with masks=True the device lists of
    ALL instances in the order of .instances [(scene_id, im_id, position in the image's list)]: .masks and .masks_visib are
    hypotheses.DeviceMasks -- .lists = (cum, offsets) is what verify.counts and maskfit.moments take as `masks` with det = the
    instance's position in .instances, and HypothesisVerifier.score takes the object itself, an estimate naming its mask by
    "instance_id" = that position.  The box of an amodal mask is the object's box clipped to the frame."""
    instances, masks, masks_visib = (), None, None


class GroundTruthInfo:
    """scene_gt_info.json's numbers (and, on request, the mask / mask_visib pairs) of a set of ground truths.
      models   {obj_id: {"vertices" (V,3), "faces" (F,3), ...}}                            (what PoseScorer takes)
      cameras  {(scene_id, im_id): {"cam_K" 9, ["depth" (H,W) z-depth in the units of the models, 0 = no measurement], ["size" (H, W)]}}
               "depth" is given for every frame or for none; without depth nothing occludes and visib_fract is the in-frame share
      delta    the tolerance of the visibility test, in the units of the models (BOP: 15 mm)
      margin   the canvas around the frame in frame sizes per side: 1.0 draws on 3H x 3W.  What lies beyond the canvas is not
               counted in px_count_all; margin 0 counts the frame only (visib_fract is then the unoccluded share of what the
               frame shows)
    .compute(gts, masks=False), gts {(scene_id, im_id): [{"obj_id", "cam_R_m2c" 9, "cam_t_m2c" 3}]} as PoseScorer takes them,
    groups the instances by (object, K), draws each group on the canvas with the keys of render.MeshRenderer (render.KeyBuffers:
    gpr_project + gpr_raster at Hc x Wc with K' = K whose principal point is moved by the frame's origin on the canvas), the views
    chunked as evaluate.vsd_errors chunks them, and classifies every pixel (gpg_classify).  A ground truth that drops a triangle
    raises ValueError, as vsd_errors does.  Per instance, in the order of gts:
      "px_count_all", "px_count_valid", "px_count_visib"    integers
      "visib_fract"      px_count_visib / px_count_all in Python, 0.0 when nothing is drawn
      "bbox_obj", "bbox_visib"      [x, y, w, h], the first may leave the frame; [-1, -1, -1, -1] when empty
      with masks=True  "mask", "mask_visib"     {"size": [H, W], "counts": [...]}: uncompressed COCO run lengths
    THE CONTRACT IS WHAT WAS DRAWN: the canvas is drawn with K' in float32, as gpr_project takes it, so its frame window need not
    equal a frame-sized render with K to the last 1/256 pixel of a projected vertex (the principal point rounds differently)."""

    def __init__(self, models, cameras, delta=15.0, margin=1.0, znear=1e-3, device="cuda"):
        who = "GroundTruthInfo"
        if math.isnan(delta):
            raise ValueError(f"{who}: delta is NaN")
        if not (margin >= 0 and math.isfinite(margin)):
            raise ValueError(f"{who}: margin must be a finite number >= 0")
        self.models, self.device = models, device
        self.delta, self.margin, self.znear = float(delta), float(margin), float(znear)
        self.table = CameraTable(who, cameras, "all_or_none")
        if self.table.H is None:
            raise ValueError(f"{who}: the frame size is unknown (no depth image and no camera 'size')")
        H, W = self.table.H, self.table.W
        self.Hc, self.Wc, self.ox, self.oy = canvas(H, W, self.margin)
        if self.Hc * self.Wc > MAX_CANVAS_PIXELS:
            raise ValueError(f"{who}: margin = {margin} gives a {self.Hc} x {self.Wc} canvas (Hc*Wc < 2^31): the largest margin "
                             f"allowed for {H} x {W} frames is {largest_margin(H, W):.3f}")

    H, W = property(lambda self: self.table.H), property(lambda self: self.table.W)

    @torch.no_grad()
    def compute(self, gts, masks=False):
        who = "GroundTruthInfo.compute"
        t, dev = self.table, self.device
        H, W, Hc, Wc = t.H, t.W, self.Hc, self.Wc
        flat, instances = [], []
        for key, listed in gts.items():
            for j, g in enumerate(listed):
                flat.append(dict(scene_id=key[0], im_id=key[1], obj_id=g["obj_id"], R=g["cam_R_m2c"], t=g["cam_t_m2c"]))
                instances.append((int(key[0]), int(key[1]), j))
        groups = grouped(who, flat, t, self.models)
        need_gpu(who, dev)
        E = len(flat)
        depth = t.depth_on(dev)
        step = render.views_step(None, Hc, Wc)
        info = torch.zeros(E, INFO, dtype=torch.int64, device=dev)
        box = torch.zeros(E, BOX, dtype=torch.int32, device=dev)
        status, clipped = torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
        lists = []                                               # per chunk: (indices, [(counts, cum, offsets) of which = 0, 1])
        for (obj, kbytes), idx in groups:
            m = self.models[obj]
            vertices, faces = _lib.upload(who, dev, _lib.checked(m["vertices"], torch.float32, (None, 3), who, "vertices"),
                                          _lib.checked(m["faces"], torch.int32, (None, 3), who, "faces"))
            K = np.frombuffer(kbytes, np.float64).copy()
            ray = torch.from_numpy(ray_map(K, H, W)[None]).to(dev)
            K[2], K[5] = K[2] + self.ox, K[5] + self.oy
            K9 = render._k9(K)
            poses = np.stack([pose_matrix(flat[i]["R"], flat[i]["t"]) for i in idx]).astype(np.float32)
            buffers = render.KeyBuffers(min(len(idx), step), vertices.shape[0], faces.shape[0], Hc, Wc, dev)
            for _, a, b in _lib.chunked(len(idx), step):
                sel = torch.as_tensor(idx[a:b], dtype=torch.int64, device=dev)
                dropped = torch.empty(b - a, dtype=torch.int32, device=dev)
                keys = buffers.draw(vertices, faces, torch.from_numpy(poses[a:b]).to(dev), K9, self.znear, dropped)[0]
                frame = None if depth is None else torch.tensor([t.index[instances[i][:2]] for i in idx[a:b]], dtype=torch.int32, device=dev)
                cls, info[sel], box[sel], status[sel] = classify(keys, (self.ox, self.oy), depth, frame, ray,
                                                                 torch.zeros(b - a, dtype=torch.int32, device=dev), self.delta)
                clipped[sel] = dropped
                if masks:
                    lists.append((idx[a:b], [encode_runs(cls, which) for which in (0, 1)]))
        info_h, box_h, status_h, clipped_h = (x.cpu().numpy() for x in (info, box, status, clipped))
        bad = np.flatnonzero(clipped_h)
        if len(bad):
            raise ValueError(f"{who}: ground truth {instances[bad[0]]} drops {int(clipped_h[bad[0]])} triangles (a vertex behind znear = "
                             f"{self.znear}, beyond 16384 px or not finite): there is no near-plane clipping")
        if status_h.any():
            raise _lib.GigaPoseHipError(f"{who}: gpg_classify reports status {int(status_h.max())} (an index outside its stack)")
        out = GroundTruthTable()
        out.instances = instances
        rows = []
        for i, (s, im, j) in enumerate(instances):
            px_all, _, px_valid, px_visib = (int(v) for v in info_h[i])
            row = dict(px_count_all=px_all, px_count_valid=px_valid, px_count_visib=px_visib,
                       visib_fract=px_visib / px_all if px_all else 0.0, bbox_obj=box_xywh(box_h[i, :4]), bbox_visib=box_xywh(box_h[i, 4:]))
            rows.append(row)
            out.setdefault((s, im), []).append(row)
        for key in gts:
            out.setdefault((int(key[0]), int(key[1])), [])
        if masks:
            both = [_in_order([(idx, parts[which]) for idx, parts in lists], E, dev) for which in (0, 1)]
            frame_box = np.stack([np.clip(box_h[:, 0], 0, W - 1), np.clip(box_h[:, 1], 0, H - 1), np.clip(box_h[:, 2], 0, W - 1), np.clip(box_h[:, 3], 0, H - 1)], axis=1)
            out.masks, out.masks_visib = (
                DeviceMasks((cum, offsets), info_h[:, count], np.where(info_h[:, count:count + 1] > 0, corners, (W, H, -1, -1)), (H, W))
                for (_, cum, offsets), count, corners in zip(both, (PX_FRAME, PX_VISIB), (frame_box, box_h[:, 4:])))
            for name, (counts, _, offsets) in zip(("mask", "mask_visib"), both):
                counts_h, offsets_h = counts.cpu().numpy(), offsets.cpu().numpy()
                for i, row in enumerate(rows):
                    row[name] = {"size": [H, W], "counts": counts_h[offsets_h[i]:offsets_h[i + 1]].tolist()}
        return out


def _in_order(chunks, E, device):
    """[(the instances' indices, (counts, cum, offsets) of one encode_runs call)] -> the lists of all E instances in index order,
    gathered on the device."""
    runs = torch.zeros(E, dtype=torch.int64, device=device)
    start = torch.zeros(E, dtype=torch.int64, device=device)    # of an instance's slice in the concatenation of the chunks' lists
    base = 0
    for idx, (counts, _, offsets) in chunks:
        sel = torch.as_tensor(idx, dtype=torch.int64, device=device)
        runs[sel] = (offsets[1:] - offsets[:-1]).to(torch.int64)
        start[sel] = offsets[:-1].to(torch.int64) + base
        base += counts.shape[0]
    offsets = torch.zeros(E + 1, dtype=torch.int64, device=device)
    offsets[1:] = torch.cumsum(runs, 0)
    if base >= 2 ** 31:
        raise ValueError(f"GroundTruthInfo.compute: {base} runs in all (the lists are indexed with 32 bits: compute fewer images per call)")
    if not chunks:
        empty = torch.zeros(0, dtype=torch.int32, device=device)
        return empty, empty.clone(), offsets.to(torch.int32)
    source = torch.arange(base, device=device) + torch.repeat_interleave(start - offsets[:-1], runs, output_size=base)
    counts = torch.cat([c for _, (c, _, _) in chunks])[source]
    cum = torch.cat([c for _, (_, c, _) in chunks])[source]
    return counts, cum, offsets.to(torch.int32)


def with_visibility(gts, info):
    """gts {(scene_id, im_id): [ground truths]} and compute()'s result -> a new gts dict whose entries are copies that carry
    "visib_fract": what PoseScorer(min_visib=...) and AddScorer(min_visib=...) read."""
    out = {}
    for key, listed in gts.items():
        rows = info[(int(key[0]), int(key[1]))]
        if len(rows) != len(listed):
            raise ValueError(f"with_visibility: image {key} lists {len(listed)} ground truths and the info {len(rows)}")
        out[key] = [dict(g, visib_fract=float(r["visib_fract"])) for g, r in zip(listed, rows)]
    return out
