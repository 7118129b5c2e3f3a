"""Inputs for the tests of the silhouette fit (gigapose_amd/maskfit.py, gigapose_testing/maskfit_ref.py), shared by the CPU and
the GPU suite.  The scene is refine_cases' (three boxes, 96 x 128) with verify_cases' masks: the silhouette at the ground truth.
Added here: starts whose out-of-plane rotation is right (what a silhouette's moments can mend), the starts that lie outside the
depth refiner's gate, small masks for the closed-form moments, and planted rows for the step."""
import functools

import numpy as np

from gigapose_amd.ingest import mask_to_rle_counts
from gigapose_amd.refine import projected_boxes

from . import maskfit_ref, raster_ref, refine_ref
from . import refine_cases as rc
from . import verify_cases as vc

H, W, K = rc.H, rc.W, rc.K
ITERS, MIN_POINTS, ELONGATION, GAIN, MARGIN = 8, 32, 0.1, 1.0, 16
GTS = vc.GTS
Z = [0, 0, 1]


def fit_starts(gt):
    """Three starts whose out-of-plane rotation is the ground truth's: turned in the plane and shifted."""
    return np.stack([rc.moved(gt, Z, 10, (6, -4, 0)), rc.moved(gt, Z, 0, (0, 0, 48)), rc.moved(gt, Z, -20, (-8, 5, -40))])


def stage_starts(gt=rc.GT):
    """Four starts about GT that the depth refiner alone leaves where they are: beyond its gate."""
    return np.stack([rc.moved(gt, Z, 0, (0, 0, 48)), rc.moved(gt, Z, -20, (-8, 5, -40)), rc.moved(gt, [2, -1, 1], 8, (10, -8, 60)),
                     rc.moved(gt, [2, -1, 1], 15, (8, -8, 70))])


def mask_box(mask):
    ys, xs = np.nonzero(mask)
    return (xs.min(), ys.min(), xs.max(), ys.max()) if len(xs) else (mask.shape[1], mask.shape[0], -1, -1)


def boxes(poses, which, margin=MARGIN):
    """MaskRefiner's default box: the start's projected box joined with the mask's box, both padded by `margin` (an integer)."""
    v, _ = rc.mesh("boxes")
    b = projected_boxes(v, poses, np.tile(K, (len(poses), 1)), H, W, margin)
    m = mask_box(vc.truth(which)["mask"])
    m = (max(m[0] - margin, -1), max(m[1] - margin, -1), min(m[2] + margin, W), min(m[3] + margin, H))
    return np.stack([np.minimum(b[:, 0], m[0]), np.minimum(b[:, 1], m[1]), np.maximum(b[:, 2], m[2]), np.maximum(b[:, 3], m[3])], axis=1).astype(np.int32)


def fit(poses, which, variant=None, iters=ITERS):
    """The restatement's loop on instance `which` from `poses`."""
    v, f = rc.mesh("boxes")
    n = len(poses)
    return maskfit_ref.refine(v, f, poses, np.tile(K, (n, 1)), [vc.truth(which)["runs"]], np.zeros(n, np.int32), boxes(poses, which), iters, MIN_POINTS,
                              ELONGATION, GAIN, H, W, variant=variant)


@functools.lru_cache(maxsize=None)
def run(which, kind, variant=None):
    """Cached: `kind` is "fit" (fit_starts), "right" (rc.starts), "wrong" (rc.wrong_starts) or "stage" (stage_starts, which = 0)."""
    gt = GTS[which]
    p = dict(fit=fit_starts, right=rc.starts, wrong=rc.wrong_starts, stage=stage_starts)[kind](gt)
    return p, fit(p, which, variant)


def depth_refined(poses, which=0):
    """refine_ref.refine with the refine tests' settings (whole frame, gate 30) from `poses` -> poses."""
    v, f = rc.mesh("boxes")
    n = len(poses)
    out = refine_ref.refine(v, f, poses, np.tile(K, (n, 1)), vc.truth(which)["depth"][None], np.zeros(n, np.int32), rc.whole_frame(n), np.full(n, rc.GATE),
                            np.full(n, rc.SCALE), rc.ITERS, rc.STEP["min_points"], rc.STEP["min_pivot"], rc.STEP["damping"], rc.STEP["tol2"], H, W)
    return out["poses"]


def iou(score, best=True):
    s = np.asarray(score, np.float64).reshape(-1, 4)
    return s[:, 0] / s[:, 1] if best else s[:, 2] / s[:, 3]


# ------------------------------------------------------------------------------------------------ small masks
def host_masks():
    """(name, dense mask (h,w) bool) for the closed-form moments; the runs are mask_to_rle_counts' (column-major)."""
    out = [("empty", np.zeros((5, 7), bool)), ("full", np.ones((5, 7), bool))]
    for name, (y, x) in (("corner 00", (0, 0)), ("corner top right", (0, 6)), ("corner bottom left", (4, 0)), ("corner bottom right", (4, 6))):
        m = np.zeros((5, 7), bool)
        m[y, x] = True
        out.append((name, m))
    m = np.zeros((5, 7), bool)
    m[2:, 3] = True                                   # a run that ends exactly at a column's end
    out.append(("ends at a column's end", m))
    m = np.zeros((5, 7), bool)
    m[3:, 1], m[:, 2], m[:2, 3] = True, True, True    # one run over three columns
    out.append(("wraps three columns", m))
    m = np.zeros((5, 7), bool)
    m[4, 1], m[:, 2:5], m[0, 5] = True, True, True    # head, three full columns, tail
    out.append(("wraps five columns", m))
    rs = np.random.RandomState(3)
    out.append(("random", rs.uniform(size=(37, 23)) > 0.6))
    return out


def zero_length_runs():
    """A list with zero-length runs of both kinds over a 5 x 7 frame, and its dense mask."""
    runs = np.asarray([0, 3, 0, 2, 4, 0, 0, 6, 20], np.int32)         # ones: [0,3) [3,5) (after a zero run of zeros), [9,9), [9,15)
    assert runs.sum() == 35
    flat = np.zeros(35, bool)
    flat[0:5], flat[9:15] = True, True
    return runs, flat.reshape(7, 5).T.copy()


def dense_sums(mask):
    """Sums over the dense mask in Python integers."""
    ys, xs = np.nonzero(mask)
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    return [len(xs), sum(xs), sum(ys), sum(x * x for x in xs), sum(x * y for x, y in zip(xs, ys)), sum(y * y for y in ys)]


# ------------------------------------------------------------------------------------------------ planted rows
EXACT_K = np.asarray([128.0, 0.0, 64.0, 0.0, 128.0, 48.0, 0.0, 0.0, 1.0])


def moments_of(n, mx, my, uxx, uxy, uyy):
    """A row of six integer sums with the given (dyadic) mean and central second moments: Sx = n*mx ...  Exact when the values
    have few bits and n is a power of two."""
    row = [n, n * mx, n * my, n * (uxx + mx * mx), n * (uxy + mx * my), n * (uyy + my * my)]
    assert all(float(v) == int(v) for v in row), row
    return [int(v) for v in row]


def planted_row(six, inter=0, edge=0):
    row = np.zeros(16, np.int64)
    row[:6], row[6], row[7] = six, inter, edge
    return row


def exact_pose():
    return rc.rigid([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (8.0, -4.0, 256.0))


def shape(n, mx, my, a, b, tr):
    """Six sums with mean (mx, my) and a = uxx - uyy, b = 2 uxy, tr = uxx + uyy."""
    return moments_of(n, mx, my, (tr + a) / 2, b / 2, (tr - a) / 2)


def planted():
    """A batch of pairs with a script of rows per call of the step (calls 0, 1, 2 and the last, judging one), and how each must
    end.  -> dict(mm (D,8), det (N), K (N,9), start (N,4,4), calls = [(rows (N,16), status (N), clipped (N))] * 4,
    want_bits (N), want_best (N), names)."""
    B, NM, F, C, R, NI = (maskfit_ref.BAD_MASK, maskfit_ref.NO_MASK, maskfit_ref.FEW, maskfit_ref.CLIPPED, maskfit_ref.ROUND, maskfit_ref.NOT_IMPROVED)
    big = 2 ** 20
    masks = [shape(1200, 66, 50, 38, 20, 110), shape(31, 66, 50, 38, 20, 110), shape(big, 66, 50, 38, 20, 110)]
    D0 = shape(1000, 60, 45, 40, 10, 100)
    round_d = shape(1000, 60, 45, 1, 0, 100)
    few = shape(31, 60, 45, 40, 10, 100)

    def seq(inters, six=D0, edges=(0, 0, 0, 0)):
        return [(six, i, e, 0, 0) for i, e in zip(inters, edges)]

    pairs = [  # name, det, [(six, inter, edge, clipped, status)] * 4, final bits, best iteration
        ("the best is kept, not the last", 0, seq((500, 800, 700, 600)), 0, 1),
        ("an exact tie keeps the earlier", 0, [(shape(1000, 60, 45, 40, 10, 100), 500, 0, 0, 0), (shape(800, 60, 45, 40, 10, 100), 800, 0, 0, 0),
                                                (shape(2800, 60, 45, 40, 10, 100), 1600, 0, 0, 0), (D0, 100, 0, 0, 0)], 0, 1),
        ("one part in 2^40 better", 2, [(shape(big, 60, 45, 40, 10, 100), big // 2, 0, 0, 0), (shape(big - 1, 60, 45, 40, 10, 100), big - 1, 0, 0, 0),
                                         (shape(big + 1, 60, 45, 40, 10, 100), big, 0, 0, 0), (shape(big - 1, 60, 45, 40, 10, 100), big - 1, 0, 0, 0)], 0, 2),
        ("one part in 2^40 worse", 2, [(shape(big, 60, 45, 40, 10, 100), big // 2, 0, 0, 0), (shape(big + 1, 60, 45, 40, 10, 100), big, 0, 0, 0),
                                        (shape(big - 1, 60, 45, 40, 10, 100), big - 1, 0, 0, 0), (shape(big, 60, 45, 40, 10, 100), big // 2, 0, 0, 0)], 0, 1),
        ("the last call is judged too", 0, seq((500, 400, 300, 900)), 0, 3),
        ("never better", 0, seq((500, 400, 300, 200)), NI, 0),
        ("a better pose on the box's edge is not kept", 0, seq((500, 800, 600, 400), edges=(0, 3, 0, 0)), 0, 2),
        ("the start counts whatever its edge", 0, seq((500, 400, 300, 200), edges=(5, 0, 0, 0)), NI, 0),
        ("few drawn pixels", 0, seq((20, 20, 20, 20), six=few), F | NI, 0),
        ("few mask pixels", 1, seq((20, 20, 20, 20)), F | NI, 0),
        ("few drawn pixels at call 2", 0, [(D0, 500, 0, 0, 0), (D0, 800, 0, 0, 0), (few, 20, 0, 0, 0), (D0, 900, 0, 0, 0)], F | NI, 0),
        ("clipped at call 1", 0, [(D0, 500, 0, 0, 0), (D0, 800, 0, 7, 0), (D0, 900, 0, 0, 0), (D0, 900, 0, 0, 0)], C | NI, 0),
        ("clipped at the last call", 0, [(D0, 500, 0, 0, 0), (D0, 800, 0, 0, 0), (D0, 900, 0, 0, 0), (D0, 950, 0, 1, 0)], C | NI, 0),
        ("no mask", -1, [((0,) * 6, 0, 0, 0, NM)] * 4, NM | NI, 0),
        ("a bad mask", 0, [((0,) * 6, 0, 0, 0, B)] * 4, B | NI, 0),
        ("det beyond the masks", 3, seq((500, 800, 700, 600)), B | NI, 0),
        ("a negative det with a clean status", -5, seq((500, 800, 700, 600)), NM | NI, 0),
        ("a bad mask and clipped", 0, [((0,) * 6, 0, 0, 2, B)] * 4, B | C | NI, 0),
        ("no mask and clipped", -1, [((0,) * 6, 0, 0, 2, NM)] * 4, NM | C | NI, 0),
        ("round, improved", 0, seq((500, 800, 700, 600), six=round_d), R, 1),
        ("round, not improved", 0, seq((500, 400, 300, 200), six=round_d), R | NI, 0),
        ("round at call 1 only", 0, [(D0, 500, 0, 0, 0), (round_d, 800, 0, 0, 0), (D0, 700, 0, 0, 0), (D0, 100, 0, 0, 0)], 0, 1),
    ]
    n = len(pairs)
    calls = []
    for c in range(4):
        rows = np.stack([planted_row(p[2][c][0], p[2][c][1], p[2][c][2]) for p in pairs])
        calls.append((rows, np.asarray([p[2][c][4] for p in pairs], np.int32), np.asarray([p[2][c][3] for p in pairs], np.int32)))
    mm = np.zeros((len(masks), 8), np.int64)
    mm[:, :6] = masks
    rs = np.random.RandomState(9)
    start = np.stack([rc.moved(rc.GT, [1, 2, 3], rs.uniform(-30, 30), rs.uniform(-20, 20, 3)) for _ in range(n)])
    return dict(mm=mm, det=np.asarray([p[1] for p in pairs], np.int32), K=np.tile(K, (n, 1)), start=start, calls=calls,
                want_bits=np.asarray([p[3] for p in pairs], np.int32), want_best=np.asarray([p[4] for p in pairs], np.int32), names=[p[0] for p in pairs])


def run_planted(p, update, variant=None):
    """The four calls of planted() through `update` (maskfit_ref.update's signature) -> (poses, state dict) after every call."""
    poses, st, out = p["start"].copy(), maskfit_ref.new_state(len(p["start"])), []
    for it, (rows, status, clipped) in enumerate(p["calls"]):
        poses, _, st = update(rows, status, p["mm"], p["det"], clipped, p["K"], p["start"], it, it == 3, MIN_POINTS, ELONGATION, GAIN, poses, st, variant)
        out.append((poses, st))
    return out
