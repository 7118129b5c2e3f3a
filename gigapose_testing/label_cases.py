"""Planted inputs for the proposal-labelling tests (tests/test_label_host.py, tests/test_gpu_label.py) and tools/probe_proposals.py:
class tokens of every kind, descriptors and banks with planted winners and ties, run-length masks at the edges of the box rule, and
boxes at the edges of the IoU test.  numpy RandomState streams only; nothing here needs a device."""
import numpy as np

from gigapose_amd.ingest import mask_to_rle_counts

from . import label_ref as ref
from . import meshes

ROW_KINDS = ("random", "massive", "constant", "nan", "inf")
EPS = 1e-6


# ------------------------------------------------------------------------------------------------ class tokens
def token_rows(seed, B, C, first_kind=0):
    """(x f32 (B, C), kinds): row b is of kind ROW_KINDS[(first_kind + b) % 5] -- random; one massive channel (1e4 beside O(1), as
    DINOv2 checkpoints have them); constant (variance 0); one NaN; one infinity."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, C)).astype(np.float32)
    kinds = [ROW_KINDS[(first_kind + b) % len(ROW_KINDS)] for b in range(B)]
    for b, kind in enumerate(kinds):
        c = int(rs.randint(C))
        if kind == "massive":
            x[b, c] = 1e4 * (1 if b % 2 else -1)
        elif kind == "constant":
            x[b] = np.float32(0.75)
        elif kind == "nan":
            x[b, c] = np.nan
        elif kind == "inf":
            x[b, c] = np.inf if b % 2 else -np.inf
    return x, kinds


def norm_parameters(seed, C, zero_beta=False):
    rs = np.random.RandomState(seed)
    gamma = (1.0 + 0.25 * rs.standard_normal(C)).astype(np.float32)
    beta = np.zeros(C, np.float32) if zero_beta else (0.1 * rs.standard_normal(C)).astype(np.float32)
    return gamma, beta


def token_layouts(x, fill=np.nan):
    """The two layouts gpa_descriptors serves, with `fill` in every element it must not read:
    "contiguous": (B, 257, C) with the class token first, strides (257 * C, 1);
    "workspace": the ViT workspace's channel-major view (C, mpad), crop b's token in column 257 * b, strides (257, mpad)."""
    B, C = x.shape
    cont = np.full((B, 257, C), fill, np.float32)
    cont[:, 0] = x
    mpad = (B * 257 + 255) // 256 * 256
    ws = np.full((C, mpad), fill, np.float32)
    ws[:, 0:B * 257:257] = x.T
    return {"contiguous": (cont, 257 * C, 1), "workspace": (ws, 257, mpad)}


# ------------------------------------------------------------------------------------------------ descriptors and banks
def unit_vectors(rs, n, C):
    v = rs.standard_normal((n, C))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def quantise(d):
    return np.rint(np.asarray(d, np.float64) * ref.Q_ONE).astype(np.int32)


def score_case(seed, P, O, T, C, plant="random"):
    """(q int32 (P, C), bank int32 (O, T, C)).  plant:
      "random"    quantised unit vectors, every proposal a noisy copy of one template
      "extreme"   every value +-2^20: the largest sums
      "ties"      an object's templates repeat (equal dots inside an object) and the objects repeat (equal obj): the first wins
      "negative"  every similarity is negative
      "corners"   the winners are planted in the first and last object and template and around multiples of 64 bank rows"""
    rs = np.random.RandomState(seed)
    bank_d = unit_vectors(rs, O * T, C).reshape(O, T, C)
    pick_o, pick_t = rs.randint(O, size=P), rs.randint(T, size=P)
    if plant == "corners":
        rows = sorted({r for r in (0, O * T - 1, 63, 64, 65, 127, 128, O * T // 2) if 0 <= r < O * T})
        flat = np.asarray([rows[p % len(rows)] for p in range(P)], np.int64)
        pick_o, pick_t = flat // T, flat % T
    noise = unit_vectors(rs, P, C)
    q_d = bank_d[pick_o, pick_t] + 0.3 * noise if P else np.zeros((0, C))
    q_d = q_d / np.maximum(np.linalg.norm(q_d, axis=1, keepdims=True), 1e-30)
    q, bank = quantise(q_d), quantise(bank_d)
    if plant == "extreme":
        q = np.where(rs.randint(2, size=(P, C)) > 0, ref.Q_ONE, -ref.Q_ONE).astype(np.int32)
        bank = np.where(rs.randint(2, size=(O, T, C)) > 0, ref.Q_ONE, -ref.Q_ONE).astype(np.int32)
        if P:
            bank[0, 0] = -q[0]                              # -C * 2^40 exactly
            bank[O - 1, T - 1] = q[0]                       # C * 2^40 (a bank of one template keeps this one)
    elif plant == "ties":
        if T >= 2:
            bank[:, T - T // 2:] = bank[:, :T // 2]         # the last T // 2 templates of every object repeat its first ones
        if O >= 2:
            bank[O - O // 2:] = bank[:O // 2]               # and the last O // 2 objects repeat the first ones
    elif plant == "negative":
        base = unit_vectors(rs, 1, C)[0]
        unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
        bank = quantise(unit(base + 0.2 * bank_d))
        q = quantise(unit(-(base + 0.2 * noise))) if P else q
    return q, bank


# every size of the issue at least once, and the pairs that matter (P, O * T around one tile; T around k)
SCORE_SHAPES = [(0, 1, 1, 64, 1), (1, 1, 1, 64, 1), (1, 2, 4, 64, 5), (63, 1, 5, 64, 5), (64, 2, 6, 384, 5), (65, 41, 4, 64, 7),
                (1, 41, 42, 1024, 5), (65, 2, 65, 384, 7), (64, 1, 65, 64, 1), (63, 41, 6, 384, 1), (65, 2, 42, 1024, 7), (2, 41, 65, 64, 5),
                (64, 1, 64, 64, 5), (65, 1, 1, 64, 7), (5, 2, 32, 64, 5), (3, 3, 43, 64, 64)]
SCORE_PLANTS = ("random", "extreme", "ties", "negative", "corners")


# ------------------------------------------------------------------------------------------------ run-length masks
def pack(lists):
    offsets = np.cumsum([0] + [len(c) for c in lists]).astype(np.int32)
    counts = np.concatenate([np.asarray(c, np.int32) for c in lists]) if lists else np.zeros(0, np.int32)
    return counts, offsets


def planted_masks(H, W):
    """Dense masks (n, H, W) bool at the edges of the box rule, and their names."""
    out = []

    def add(name, fill):
        m = np.zeros((H, W), bool)
        fill(m)
        out.append((name, m))

    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        add(f"one pixel at ({y}, {x})", lambda m, y=y, x=x: m.__setitem__((y, x), True))
    add("whole frame", lambda m: m.__setitem__(slice(None), True))
    add("empty", lambda m: None)
    add("first column (first run of length 0)", lambda m: m.__setitem__((slice(None), 0), True))
    add("a block", lambda m: m.__setitem__((slice(H // 4, H // 2 + 1), slice(W // 4, W // 2 + 1)), True))

    def crossing(m, tail):
        # one run from the middle of column W // 2 that ends `tail` pixels into the next column (0: exactly on the boundary)
        flat = np.zeros(H * W, bool)
        a = (W // 2) * H + H // 2
        flat[a:(W // 2 + 1) * H + tail] = True
        m[:] = flat.reshape(W, H).T

    if W >= 2:
        add("a run ending exactly on a column boundary", lambda m: crossing(m, 0))
        add("a run ending one pixel past a column boundary", lambda m: crossing(m, 1))
    add("scattered", lambda m: m.__setitem__((slice(H // 3, None, 5), slice(W // 5, None, 3)), True))
    return [n for n, _ in out], np.stack([m for _, m in out])


def mask_lists(masks):
    return [mask_to_rle_counts(m) for m in masks]


def dense_boxes(masks):
    """numpy.nonzero's reading: (box int32 (n,4) x0 y0 x1 y1 exclusive, area int64 (n)); an empty mask gives zeros."""
    box, area = np.zeros((len(masks), 4), np.int32), np.zeros(len(masks), np.int64)
    for n, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            box[n], area[n] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1), len(ys)
    return box, area


def decode(counts, H, W):
    """A run list -> the dense (H, W) bool mask, by the format's parity rule."""
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(bool)
    return flat.reshape(W, H).T


# ------------------------------------------------------------------------------------------------ boxes for the NMS
THRESHOLD_PAIRS = {            # against A = (0, 0, 5, 1), IoU threshold 1 / 4: inter = 2
    "at": (3, 0, 8, 1),        # union 8: 2 * 4 == 8 -> kept (the comparison is strict)
    "above": (3, 0, 7, 1),     # union 7: suppressed
    "below": (3, 0, 9, 1),     # union 9: kept
}


def chain(P, y=0):
    """P boxes of width 6 at steps of 3: each overlaps only its neighbours, at IoU 3 / 9 > 1 / 4.  Greedy keeps 0, 2, 4, ..: a
    suppressed box suppresses nothing, across every 64-bit word boundary."""
    x = 3 * np.arange(P)
    return np.stack([x, np.full(P, y), x + 6, np.full(P, y + 1)], axis=1).astype(np.int32)


def nms_case(seed, P):
    """(box int32 (P,4), label int32 (P)): clusters of jittered boxes, degenerate (empty and inverted) boxes, the three threshold
    pairs in front and a chain of up to 70 boxes at the end, which crosses the last word boundaries."""
    rs = np.random.RandomState(seed)
    centres = rs.randint(0, 400, size=(max(1, P // 6), 2))
    c = centres[rs.randint(len(centres), size=P)]
    wh = rs.randint(8, 40, size=(P, 2))
    jit = rs.randint(-6, 7, size=(P, 2))
    box = np.concatenate([c + jit, c + jit + wh], axis=1).astype(np.int32)
    n = 0
    for b in [(0, 0, 5, 1)] + list(THRESHOLD_PAIRS.values()) + [(7, 7, 7, 30), (9, 9, 4, 4), (0, 0, 0, 0)]:
        if n < P // 2:
            box[n] = np.asarray(b) + (1000 + 20 * (n > 3) * n, 1000, 1000 + 20 * (n > 3) * n, 1000)
            n += 1
    m = min(P - n, 70)
    if m > 0:
        box[P - m:] = chain(m, y=2000)
    label = rs.randint(0, 3, size=P).astype(np.int32)
    return box, label


# ------------------------------------------------------------------------------------------------ the end-to-end objects
def golden_meshes():
    """What tests/golden/label_meshes.npz holds: {name_vertices, name_faces, name_colours} of "boxes" (meshes.three_boxes) and
    "ball" (a squashed icosphere: every view differs).  The end-to-end test reads the file; the host tests hold it to this."""
    out = {}
    v, f, c = meshes.icosphere(2, 0.7)
    ball = ((v * np.asarray([1.0, 0.8, 0.6], np.float32)).astype(np.float32), f, c)
    for name, (v, f, c) in (("boxes", meshes.three_boxes()), ("ball", ball)):
        out[f"{name}_vertices"], out[f"{name}_faces"], out[f"{name}_colours"] = v, f, c
    return out
