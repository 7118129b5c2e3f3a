"""Planted inputs for the appearance tests (tests/test_appear_host.py, tests/test_gpu_appear.py) and tools/probe_appearance.py: patch
tokens of every kind in the two layouts gpp_patch_descriptors serves, crop masks at the edges of the occupancy rule, and limb
tensors with planted maxima, ties, negative rows, invalid winners and the extremes of the limb ranges.  numpy RandomState streams
only; nothing here needs a device."""
import numpy as np

from . import appear_ref as ref
from . import label_cases

EPS = label_cases.EPS
T = 257                                                     # tokens of a crop: the class token, then 256 patches


# ------------------------------------------------------------------------------------------------ patch tokens
def patch_tokens(seed, B, C, first_kind=0):
    """(x f32 (B, 256, C), kinds (B * 256)): token (b, n) is of kind ROW_KINDS[(first_kind + 256 b + n) % 5] of label_cases.token_rows
    -- random, one massive channel, constant, one NaN, one infinity."""
    x, kinds = label_cases.token_rows(seed, B * ref.PATCHES, C, first_kind)
    return x.reshape(B, ref.PATCHES, C), kinds


def token_layouts(x, fill=np.nan):
    """The two layouts with `fill` in every element that must not be read -> {name: (store, offset, crop_stride, token_stride, channel_stride)}:
    "contiguous": (B, 257, C), the class token first; "workspace": the ViT workspace's channel-major view (C, mpad), token n of crop
    b in column 257 * b + 1 + n, the columns from 257 * B on padding."""
    B, _, C = x.shape
    cont = np.full((B, T, C), fill, np.float32)
    cont[:, 1:] = x
    mpad = (B * T + 255) // 256 * 256
    ws = np.full((C, mpad), fill, np.float32)
    for b in range(B):
        ws[:, T * b + 1:T * (b + 1)] = x[b].T
    return {"contiguous": (cont, C, T * C, C, 1), "workspace": (ws, 1, T, 1, mpad)}


# ------------------------------------------------------------------------------------------------ crop masks
PLANTED_COUNTS = (0, 97, 98, 99, 196)
PLANTED_PATCHES = (0, 15, 240, 255, 119)                    # the first, the corners, the last, one inside


def planted_masks(B, seed=0):
    """(mask f32 (B, 224, 224), planted): crop b holds random blobs, and in patch PLANTED_PATCHES[k] exactly PLANTED_COUNTS[(k + b) % 5]
    set pixels (the rest of the cell 0.5 exactly -- not set -- NaN, or 0.25); planted = {(b, patch): count}.  Set pixels are 1.0 or 0.75."""
    rs = np.random.RandomState(1000 + seed)
    mask = np.zeros((B, 224, 224), np.float32)
    planted = {}
    for b in range(B):
        yy, xx = np.mgrid[0:224, 0:224]
        for _ in range(3):
            cy, cx, ry, rx = rs.uniform(30, 194), rs.uniform(30, 194), rs.uniform(10, 80), rs.uniform(10, 80)
            mask[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1.0
        for k, patch in enumerate(PLANTED_PATCHES):
            count = PLANTED_COUNTS[(k + b) % len(PLANTED_COUNTS)]
            py, px = divmod(patch, ref.SIDE)
            cell = np.asarray([0.5, np.nan, 0.25], np.float32)[rs.randint(3, size=ref.CELL * ref.CELL)]
            cell[rs.permutation(ref.CELL * ref.CELL)[:count]] = np.asarray([1.0, 0.75], np.float32)[rs.randint(2, size=count)]
            mask[b, ref.CELL * py:ref.CELL * (py + 1), ref.CELL * px:ref.CELL * (px + 1)] = cell.reshape(ref.CELL, ref.CELL)
            planted[(b, patch)] = count
    return mask, planted


# ------------------------------------------------------------------------------------------------ limbs with planted answers
def quantised_units(rs, shape_rows, C):
    return label_cases.quantise(label_cases.unit_vectors(rs, int(np.prod(shape_rows)), C)).reshape(tuple(shape_rows) + (C,))


PLANTED_MAX_AT = (0, 15, 16, 255)                           # template patches that hold the maximum of one query patch each
TIE_TILES, TIE_LANES = (3, 35), (5, 6, 9)                   # equal maxima in two 16-column tiles; in one tile (two registers, two lane groups)
INVALID_WINNER = 100                                        # an invalid template patch with the largest dot
ONE_QUERY, ONE_TEMPLATE = 77, 200


def planted_pairs(seed, C):
    """Four query crops and four bank rows of quantised unit vectors, as limbs, with every planted answer in (crop 0, row 0):
      crop 0  ~60 % valid; its first 7 valid patches i0 .. i6 are copied into row 0: i0 .. i3 -> PLANTED_MAX_AT; i4 -> both TIE_TILES;
              i5 -> the three TIE_LANES; i6 -> INVALID_WINNER, which is not valid
      crop 1  exactly one valid patch (ONE_QUERY);   crop 2  no valid patch;   crop 3  all valid, base + noise
      row 0   ~60 % valid + the plants;   row 1  exactly one valid patch (ONE_TEMPLATE);   row 2  none;   row 3  -(base + noise): all dots negative
    -> dict(qa int8 (3, 4, 256, C), q_valid u8 (4, 256), ta, t_valid, plants = the patches i0 .. i6)."""
    rs = np.random.RandomState(seed)
    U, V = quantised_units(rs, (4, ref.PATCHES), C), quantised_units(rs, (4, ref.PATCHES), C)
    base = label_cases.unit_vectors(rs, 1, C)[0]
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    U[3] = label_cases.quantise(unit(base + 0.2 * label_cases.unit_vectors(rs, ref.PATCHES, C)))
    V[3] = label_cases.quantise(unit(-(base + 0.2 * label_cases.unit_vectors(rs, ref.PATCHES, C))))
    q_valid = (rs.uniform(size=(4, ref.PATCHES)) < 0.6).astype(np.uint8)
    t_valid = (rs.uniform(size=(4, ref.PATCHES)) < 0.6).astype(np.uint8)
    q_valid[1], q_valid[2], q_valid[3] = 0, 0, 1
    q_valid[1, ONE_QUERY] = 1
    t_valid[1], t_valid[2], t_valid[3] = 0, 0, 1
    t_valid[1, ONE_TEMPLATE] = 3                             # any non-zero byte is valid
    plants = np.flatnonzero(q_valid[0])[:7]
    targets = [(j,) for j in PLANTED_MAX_AT] + [TIE_TILES, TIE_LANES, (INVALID_WINNER,)]
    for i, js in zip(plants, targets):
        for j in js:
            V[0, j], t_valid[0, j] = U[0, i], 1
    t_valid[0, INVALID_WINNER] = 0
    return dict(qa=ref.q_to_limbs(U), q_valid=q_valid, ta=ref.q_to_limbs(V), t_valid=t_valid, plants=plants)


def all_pairs_with_bad(Bq, R):
    """Every (crop, row) pair, with the bad indices -1, Bq and R in between -> (qi, ti) int32."""
    qi, ti = [], []
    for q in range(Bq):
        for t in range(R):
            qi.append(q), ti.append(t)
        qi.append((-1, Bq, q, q)[q % 4]), ti.append((0, 0, -1, R)[q % 4])
    return np.asarray(qi, np.int32), np.asarray(ti, np.int32)


def extreme_limbs(seed, rows, C):
    """int8 (3, rows, 256, C) with every limb at an extreme of its range, either sign: a0, a1 in {-64, 63}, a2 in {-64, 64}.  Patch 0 of
    row 0 is all -64 (against itself every product is 4096: the accumulator of weight 2 reaches 3 * 4096 * C, the header's bound at
    C = 2048), patch 1 of row 0 is (-64, -64, 64)."""
    rs = np.random.RandomState(seed)
    a = np.where(rs.randint(2, size=(3, rows, ref.PATCHES, C)) > 0, np.int8(-64), np.int8(63)).astype(np.int8)
    a[2][a[2] == 63] = 64
    a[:, 0, 0] = -64
    a[:, 0, 1] = -64
    a[2, 0, 1] = 64
    return a
