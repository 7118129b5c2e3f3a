"""Inputs for the tests of the detection-scoring stage (gigapose_amd/detections.py, gigapose_testing/coco_ref.py), shared by the CPU
and the GPU suite: run lists at the edges of the scan and of the search, groups of detections and ground truths at the edges of
COCO's matching rule, rankings for the AP arithmetic, and detections made from the visible masks of gtinfo_cases' small scene."""
import numpy as np

from gigapose_amd.ingest import mask_to_rle_counts

FRAMES = ((1, 1), (1, 37), (37, 1), (48, 64), (16384, 256))
RUN_COUNTS = (1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 2049)        # the wave, the thread stride and kScanChunk = 1024, each +- 1
THRESHOLDS, THR_DEN = tuple(range(10, 20)), 20


# ------------------------------------------------------------------------------------------------ run lists
def pack_cum(lists):
    """Run lists -> (cum int32 (total), offsets int32 (D+1)): what the scans leave."""
    offsets = np.cumsum([0] + [len(c) for c in lists]).astype(np.int32)
    cum = np.concatenate([np.cumsum(np.asarray(c, np.int64)) for c in lists]).astype(np.int32) if lists else np.zeros(0, np.int32)
    return cum, offsets


def decode(counts, HW):
    """A run list -> its HW pixels (column-major) as bool, by the format's parity rule."""
    flat = np.repeat(np.arange(len(counts)) & 1, np.asarray(counts, np.int64)).astype(bool)
    assert flat.size == HW
    return flat


def complement(counts):
    counts = [int(v) for v in counts]
    return counts[1:] if counts[0] == 0 and len(counts) > 1 else [0] + counts


def with_runs(HW, n, rs):
    """A list of exactly n runs over HW pixels; the runs after the first are not empty where HW allows it."""
    if n == 1:
        return [HW]
    if HW >= n:
        cuts = np.sort(rs.choice(np.arange(1, HW), n - 1, replace=False)) if HW > n else np.arange(1, n)
        return np.diff(np.concatenate(([0], cuts, [HW]))).tolist()
    lens = [0] * n                                                    # a tiny frame: zero-length runs make up the number
    lens[-1 if n % 2 == 0 else -2] = HW
    return lens


def frame_lists(H, W, seed=0):
    """(names, run lists) on an H x W frame: the format's edge cases, a mask and its complement, a mask that begins exactly where
    another one's runs end, random masks, and lists of every length of RUN_COUNTS."""
    HW, rs = H * W, np.random.RandomState(1000 + seed)
    out = [("empty: one run", [HW]), ("full: [0, HW]", [0, HW])]
    if HW > 1:
        out += [("pixel 0", [0, 1, HW - 1]), ("the last pixel", [HW - 1, 1])]
    if HW >= 8:
        a = HW // 8
        out += [("a block of runs", [a, a, a, a, HW - 4 * a]), ("begins where the block's runs end", [2 * a, a, a, a, HW - 5 * a]),
                ("ends where the block's runs begin", [0, a, a, a, HW - 3 * a])]
        if HW <= 1 << 16:
            for n in range(3):
                m = rs.uniform(size=(H, W)) < (0.1, 0.5, 0.9)[n]
                out.append((f"random {n}", mask_to_rle_counts(m).tolist()))
        for n in RUN_COUNTS:
            out.append((f"{n} runs", with_runs(HW, n, rs)))
    out += [(f"complement of {name}", complement(c)) for name, c in list(out)]
    return [n for n, _ in out], [np.asarray(c, np.int32) for _, c in out]


def every_pair(n):
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return a.reshape(-1).astype(np.int32), b.reshape(-1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ groups for the matching
def planted_groups():
    """(name, inter D x G, area_det, area_gt, ignore, dt_match at 10/20): the edges of the rule, each worked by hand."""
    lane = [0] * 65
    tie_i, tie_a = list(lane), [9] * 65
    tie_i[0], tie_a[0], tie_i[64], tie_a[64] = 1, 1, 2, 4             # area_det = 2: IoU 1/2 at g = 0, 2/4 at g = 64
    return [
        ("the threshold met exactly: 8 * 20 == 10 * 16", [[8]], [12], [12], [0], [0]),
        ("one below it: 7 * 20 < 10 * 17", [[7]], [12], [12], [0], [-1]),
        ("equal IoUs as 1/2 and 2/4 across the 64-lane stride: the last one", [tie_i], [2], tie_a, [0] * 65, [64]),
        ("an ignored ground truth of higher IoU beside a non-ignored one", [[8, 10]], [10], [10, 10], [0, 1], [0]),
        ("only an ignored candidate", [[0, 10]], [10], [10, 10], [0, 1], [1]),
        ("a detection that finds only a matched ground truth", [[10], [10]], [10, 10], [10], [0], [0, -1]),
        ("the second best is left for the second detection", [[10, 8], [10, 8]], [10, 10], [10, 10], [0, 0], [0, 1]),
        ("union 0", [[0]], [0], [0], [0], [-1]),
        ("no ground truth", [[], []], [5, 5], [], [], [-1, -1]),
        ("no detection", [], [], [7, 7], [0, 1], []),
    ]


def random_group(rs, D, G, spread=6):
    """Small integers, so that equal IoUs (as equal and as unequal fractions) are common."""
    area_det, area_gt = rs.randint(1, spread + 1, D) * 4, rs.randint(1, spread + 1, G) * 4
    inter = np.minimum(rs.randint(0, 4 * spread + 1, (D, G)), np.minimum(area_det[:, None], area_gt[None, :]))
    inter[rs.uniform(size=(D, G)) < 0.3] = 0
    ignore = (np.arange(G) >= rs.randint(0, G + 1)).astype(np.uint8)
    return inter, area_det, area_gt, ignore


def assemble(groups):
    """[(inter D x G, area_det, area_gt, ignore)] -> the flat arrays of gpc_match as a dict."""
    det_off, gt_off, pair_off, inter, ad, ag, ig = [0], [0], [], [], [], [], []
    for block, area_det, area_gt, ignore in groups:
        D, G = len(area_det), len(area_gt)
        pair_off.append(sum(len(b) for b in inter))
        inter.append(np.asarray(block, np.int64).reshape(D * G))
        det_off.append(det_off[-1] + D), gt_off.append(gt_off[-1] + G)
        ad.append(np.asarray(area_det, np.int64).reshape(D)), ag.append(np.asarray(area_gt, np.int64).reshape(G))
        ig.append(np.asarray(ignore, np.uint8).reshape(G))
    cat = lambda parts, dtype: np.concatenate(parts + [np.zeros(0, dtype)]).astype(dtype)      # noqa: E731
    return dict(det_off=np.asarray(det_off, np.int32), gt_off=np.asarray(gt_off, np.int32), pair_off=np.asarray(pair_off, np.int32),
                inter=cat(inter, np.int64), area_det=cat(ad, np.int64), area_gt=cat(ag, np.int64), gt_ignore=cat(ig, np.uint8))


MATCH_KEYS = ("det_off", "gt_off", "pair_off", "inter", "area_det", "area_gt", "gt_ignore")


def match_args(case):
    return [case[k] for k in MATCH_KEYS]


def size_groups(seed=0):
    """Random groups of G = 0, 1, 63, 64, 65, 130 by D = 0, 1, 100, 101."""
    rs = np.random.RandomState(2000 + seed)
    return [random_group(rs, D, G) for G in (0, 1, 63, 64, 65, 130) for D in (0, 1, 100, 101)]


# ------------------------------------------------------------------------------------------------ rankings for the AP
def ranking_groups(seed, n_img=4, cats=(1, 2, 5), T=3):
    """Random matched detections: groups as average_precision takes them, scores with ties, ignored detections, a category
    without ground truths and one without detections."""
    rs = np.random.RandomState(3000 + seed)
    groups = []
    for _ in range(n_img):
        for c in cats:
            D = int(rs.randint(0, 9)) if c != 5 else 0
            match = np.where(rs.uniform(size=(T, D)) < 0.6, rs.randint(0, 4, (T, D)), -1).astype(np.int32)
            ignore = ((match >= 0) & (rs.uniform(size=(T, D)) < 0.2)).astype(np.uint8)
            scores = np.sort(rs.randint(0, 6, D) / 8.0)[::-1]
            groups.append(dict(category=c, scores=scores, dt_match=match, dt_ignore=ignore, npig=int(rs.randint(0, 5))))
    groups.append(dict(category=9, scores=np.asarray([0.5, 0.25]), dt_match=np.full((T, 2), -1, np.int32), dt_ignore=np.zeros((T, 2), np.uint8), npig=0))
    return groups


def one_cell(matched, npig, scores=None, ignored=None):
    """One category, one threshold, one image: a ranking as a group list."""
    D = len(matched)
    scores = np.arange(D, 0, -1) / float(D + 1) if scores is None else np.asarray(scores, np.float64)
    return [dict(category=1, scores=scores, dt_match=np.where(np.asarray(matched, bool), 0, -1).astype(np.int32).reshape(1, D),
                 dt_ignore=np.asarray([0] * D if ignored is None else ignored, np.uint8).reshape(1, D), npig=npig)]


TOY = ([1, 0, 1], 2)          # 2 ground truths, 3 detections: hit, miss, hit.  Precisions 1, 1/2, 2/3 -> from the right 1, 2/3, 2/3;
#                               recall 1/2 from rank 0, 1 from rank 2: levels 0 .. 50 read 1, levels 51 .. 100 read 2/3:
#                               AP = (51 + 50 * 2/3) / 101 = 253 / 303


# ------------------------------------------------------------------------------------------------ detections from ground-truth masks
def shifted(counts, H, W, dx):
    """The mask of a run list moved dx columns to the right (what leaves the frame is lost) -> a run list."""
    m = decode(counts, H * W).reshape(W, H).T
    out = np.zeros_like(m)
    out[:, dx:] = m[:, :W - dx]
    return mask_to_rle_counts(out).tolist()


def tight_xywh(counts, H, W):
    m = decode(counts, H * W).reshape(W, H).T
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if len(ys) else [0, 0, 0, 0]


def detection(counts, H, W, category, score, bbox=None):
    return dict(category_id=int(category), score=float(score), bbox=tight_xywh(counts, H, W) if bbox is None else list(bbox),
                segmentation=dict(counts=[int(v) for v in counts], size=[H, W]))


def perturbed_detections(rows, categories, H, W, name="mask_visib", box="bbox_visib"):
    """From an image's ground-truth rows: every mask as a detection (its own box), then a duplicate of the first at a lower score,
    the second under a wrong category, and every mask shifted by 3 columns at a low score."""
    dets = [detection(r[name]["counts"], H, W, c, 0.9 - 0.05 * n, r[box]) for n, (r, c) in enumerate(zip(rows, categories))]
    dets.append(dict(dets[0], score=0.5))
    if len(rows) > 1:
        dets.append(dict(dets[1], category_id=categories[1] + 7, score=0.95))
    for n, (r, c) in enumerate(zip(rows, categories)):
        x, y, w, h = r[box]
        dets.append(detection(shifted(r[name]["counts"], H, W, 3), H, W, c, 0.3 - 0.01 * n, [x + 3, y, w, h]))
    return dets


def host_images(gts_rows, categories, detections, min_visib, iou_type, name="mask_visib", box="bbox_visib"):
    """{key: rows}, {key: [category]}, {key: [CNOS dicts]} -> the `images` of coco_ref.evaluate, in sorted key order."""
    def shape(x, counts, xywh):
        if iou_type == "segm":
            return dict(x, cum=np.cumsum(np.asarray(counts, np.int64)).astype(np.int32))
        return dict(x, box=[xywh[0], xywh[1], xywh[0] + xywh[2], xywh[1] + xywh[3]])

    images = []
    for key in sorted(set(gts_rows) | set(detections)):
        gts = [shape(dict(category=c, ignore=min_visib is not None and r["visib_fract"] < min_visib), r[name]["counts"], r[box])
               for r, c in zip(gts_rows.get(key, []), categories.get(key, []))]
        dets = [shape(dict(category=d["category_id"], score=d["score"]), d["segmentation"]["counts"], d["bbox"]) for d in detections.get(key, [])]
        images.append((gts, dets))
    return images
