"""CPU: the host half of ADD / ADD-S / the model diameter (gigapose_amd/distances.py, libgigapose_dist.so, include/gigapose_dist.h).

The numpy restatement of the header (gigapose_testing/dist_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_dist.py); here it is held to something that cannot share its mistakes: Python-integer arithmetic on inputs where
every operation up to v_i is exact (integer vertices, signed permutation matrices, integer translations), the rounding of the
root decided with math.isqrt.  Planted cases pin the definitions; six subtly wrong scorers fail the same checks.  Beside that:
the library against its header, the argument validation of every entry point (no GPU needed), AddScorer's host logic over the
restatement's errors against a brute-force matcher, and the nearest neighbours against scipy's cKDTree."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, distances, evaluate, ingest, onboard, render
from gigapose_testing import dist_ref
from gigapose_testing.symbols import exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the library and its header
def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gigapose_dist.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpd_[a-z0-9_]+)\s*\(", src)))


def test_dist_library_exports_exactly_its_header_and_no_symbol_of_the_other_libraries():
    names = declared_symbols()
    assert names == ["gpd_abi_version", "gpd_add", "gpd_adds", "gpd_diameter2", "gpd_last_error", "gpd_root"]
    exported = exported_symbols(distances.DIST_LIB_PATH)
    assert [n for n in exported if n.startswith("gpd_")] == names
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the dist library"
    lib = distances.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gpd_abi_version() >= 1
    from gigapose_amd import rle_strings, texture

    others = [_lib.LIB_PATH, _lib.PROBE_LIB_PATH, ingest.INGEST_LIB_PATH, onboard.ONBOARD_LIB_PATH, render.RENDER_LIB_PATH,
              evaluate.EVAL_LIB_PATH] + [os.path.join(os.path.dirname(_lib.LIB_PATH), f) for f in ("libgigapose_rlestr.so", "libgigapose_texture.so")]
    assert rle_strings and texture
    for path in others:
        assert os.path.exists(path), path
        assert not [n for n in exported_symbols(path) if n.startswith("gpd_")], path


def test_dist_argument_validation_of_the_library_needs_no_gpu():
    lib = distances.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    err = lib.gpd_last_error
    for name in ("gpd_add", "gpd_adds"):
        f = getattr(lib, name)
        tag = name.encode() + b":"
        assert f(null, 5, null, null, 3, 20, null, null, null) == -1 and tag in err() and b"null" in err()
        for kw in range(5):                                      # each pointer in turn
            args = [one] * 5
            args[kw] = null
            assert f(args[0], 5, args[1], args[2], 3, 20, args[3], args[4], null) == -1 and b"null" in err(), kw
        for V, N in ((0, 3), (-1, 3), (2 ** 20 + 1, 3), (5, 65536), (5, -1)):
            assert f(one, V, one, one, N, 20, one, one, null) == -1 and tag in err() and b"bad sizes" in err(), (V, N)
        for k in (65, -65, 2 ** 20):
            assert f(one, 5, one, one, 3, k, one, one, null) == -1 and b"k must be" in err(), k
        assert f(one, 5, one, one, 3, 20, ctypes.c_void_p(12), one, null) == -1 and b"aligned" in err()
        assert f(null, 5, null, null, 0, 20, null, null, null) == 0                  # N = 0: nothing to do
        assert f(null, 2 ** 20, null, null, 0, -64, null, null, null) == 0
        assert f(null, 5, null, null, 0, 65, null, null, null) == -1                 # ... but the arguments are still checked
    d = lib.gpd_diameter2
    assert d(null, 5, one, null) == -1 and b"gpd_diameter2" in err() and b"null" in err()
    assert d(one, 5, null, null) == -1 and b"null" in err()
    for V in (0, -3, 2 ** 20 + 1):
        assert d(one, V, one, null) == -1 and b"bad sizes" in err(), V
    assert d(one, 5, ctypes.c_void_p(12), null) == -1 and b"aligned" in err()
    r, n = lib.gpd_root, ctypes.c_longlong
    assert r(null, n(4), one, null) == -1 and b"gpd_root" in err() and b"null" in err()
    assert r(one, n(4), null, null) == -1 and b"null" in err()
    for bad in (-1, 2 ** 31, 2 ** 40):
        assert r(one, n(bad), one, null) == -1 and b"bad size" in err(), bad
    assert r(null, n(0), null, null) == 0


def test_dist_argument_validation_of_the_python_layer_needs_no_gpu():
    v, p = torch.zeros(5, 3), torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    f = distances.add_sums
    with pytest.raises(ValueError, match="vertices"):
        f(v.double(), p, p, False)
    with pytest.raises(ValueError, match="vertices"):
        f(v[:, :2], p, p, False)
    with pytest.raises(ValueError, match="must be a torch tensor"):
        f(v.numpy(), p, p, True)
    with pytest.raises(ValueError, match="est"):
        f(v, p.float(), p, False)
    with pytest.raises(ValueError, match="gt"):
        f(v, p, p[:1], False)
    with pytest.raises(ValueError, match="not contiguous"):
        f(v, p.transpose(1, 2), p, False)
    with pytest.raises(ValueError, match="V = 0"):
        f(v[:0], p, p, True)
    with pytest.raises(ValueError, match="k must be"):
        f(v, p, p, True, k=65)
    with pytest.raises(ValueError, match="k must be"):
        f(v, p, p, True, k=1.5)
    big = p[:1].expand(65536, 4, 4).contiguous()
    with pytest.raises(ValueError, match="65535"):
        f(v, big, big, False)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        f(v, p, p, False)                                                            # everything right but the device
    eye = np.eye(4)[None].repeat(2, 0)
    with pytest.raises(ValueError, match="vertices"):
        distances.add_errors(np.zeros((5, 2), np.float32), eye, eye)
    with pytest.raises(ValueError, match="gt"):
        distances.add_errors(np.zeros((5, 3), np.float32), eye, eye[:1])
    with pytest.raises(ValueError, match="dtype"):
        distances.add_errors(np.zeros((5, 3), np.int32), eye, eye)
    with pytest.raises(ValueError, match="k must be"):
        distances.add_errors(np.zeros((5, 3), np.float32), eye, eye, k=-65)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        distances.add_errors(np.zeros((5, 3), np.float32), eye, eye, device="cpu")
    with pytest.raises(ValueError, match="V = 0"):
        distances.model_diameter(np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="vertices"):
        distances.model_diameter(np.zeros((4, 4), np.float32))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        distances.model_diameter(np.zeros((4, 3), np.float32), device="cpu")
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        distances.roots(torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="no model"):
        distances.AddScorer({1: dict(vertices=v.numpy())}, [dict(scene_id=1, im_id=1, obj_id=2, inst_count=1)], {})
    with pytest.raises(ValueError, match="tau_max"):
        distances.AddScorer({1: dict(vertices=v.numpy())}, [], {}, tau_max=0.0)
    np.testing.assert_array_equal(distances.errors_from_sums([3 << 20, 7, 5], [0, 2, 0], 3, 20), [1.0, np.inf, 5 / (3 << 20)])
    np.testing.assert_array_equal(distances.errors_from_sums([3, 5], [0, 1], 4, -2), [3.0, np.inf])


# ---------------------------------------------------------------------------------------------- exact integer arithmetic
def quarter_turns():
    """The 24 rotations by multiples of 90 degrees: signed permutation matrices of determinant +1."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            R = np.zeros((3, 3))
            for i, p in enumerate(perm):
                R[i, p] = -1.0 if signs >> i & 1 else 1.0
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    return out


def rigid(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def exact_points(M, vertices):
    M = [[int(x) for x in row] for row in np.asarray(M)[:3]]
    return [tuple(sum(M[i][c] * int(p[c]) for c in range(3)) + M[i][3] for i in range(3)) for p in np.asarray(vertices)]


def exact_d2(a, b):
    return sum((x - y) ** 2 for x, y in zip(a, b))


def exact_q(v, k):
    """The half-to-even rounding of the exact sqrt(v) * 2^k for an integer v >= 0, decided with integers alone."""
    if k >= 0:
        X = v << (2 * k)                                 # sqrt(v) * 2^k = sqrt(X); X is an integer, so sqrt(X) is never f + 1/2
        f = math.isqrt(X)
        return f + (X > f * f + f)                       # sqrt(X) > f + 1/2  <=>  X > f^2 + f + 1/4
    m = -k
    f = math.isqrt(v >> (2 * m))                         # floor(sqrt(v) / 2^m)
    mid2 = (2 * f + 1) ** 2 << (2 * m - 2)               # ((f + 1/2) * 2^m)^2, an integer for m >= 1
    return f + (v > mid2 or (v == mid2 and f % 2 == 1))


def exact_sums(vertices, est, gt, symmetric, k):
    out = []
    for P, G in zip(est, gt):
        e, g = exact_points(P, vertices), exact_points(G, vertices)
        v = [min(exact_d2(gi, ej) for ej in e) for gi in g] if symmetric else [exact_d2(a, b) for a, b in zip(e, g)]
        out.append(sum(exact_q(x, k) for x in v))
    return out


def exact_diameter2(vertices):
    p = [tuple(int(c) for c in row) for row in np.asarray(vertices)]
    return max([exact_d2(p[i], p[j]) for i in range(len(p)) for j in range(i + 1, len(p))] or [0])


def key_of(x):
    return int(np.asarray([float(x)], np.float64).view(np.uint64)[0])


def integer_case():
    """37 integer vertices within +-20 (far from the origin on purpose: centred at (40, -30, 25)), 10 pairs of quarter-turn poses
    with integer translations; pair 0 has est = gt; pair 1 differs by a translation only."""
    rs = np.random.RandomState(19)
    vertices = (rs.randint(-20, 21, (37, 3)) + (40, -30, 25)).astype(np.float32)
    turns = quarter_turns()
    est = np.stack([rigid(turns[rs.randint(24)], rs.randint(-15, 16, 3)) for _ in range(10)])
    gt = np.stack([rigid(turns[rs.randint(24)], rs.randint(-15, 16, 3)) for _ in range(10)])
    gt[0] = est[0]
    gt[1] = est[1]
    gt[1, :3, 3] += (1, -2, 1)
    return vertices, est, gt


TURN_Z = rigid([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (0, 0, 0))                         # a quarter turn about z


def closed_set():
    """11 points in general position and their images under the four quarter turns about z: closed under TURN_Z."""
    rs = np.random.RandomState(23)
    base = rs.randint(1, 30, (11, 3)).astype(np.float64)
    pts = [np.linalg.matrix_power(TURN_Z[:3, :3], q) @ p for p in base for q in range(4)]
    return np.asarray(pts, np.float32)


DIRECTION_VERTICES = np.asarray([(0, 0, 0), (10, 0, 0), (0, 1, 0)], np.float32)
DIRECTION_GT = rigid(np.eye(3), (8, 0, 0))                                           # gt -> est: 2 + 8 + sqrt(5); est -> gt: 8 + 2 + 8


def last_index_case():
    """6 vertices; under est = identity, gt = a shift by (100, 0, 0), every ground-truth point's nearest estimate point is the
    LAST vertex (index 5, alone near x = 100 .. 130), the ones at indices 0..4 lie around the origin."""
    vertices = np.asarray([(0, 0, 0), (3, 1, 0), (1, 4, 2), (2, 2, 5), (4, 0, 1), (115, 2, 2)], np.float32)
    return vertices, np.eye(4)[None], rigid(np.eye(3), (100, 0, 0))[None]


class Scorer:
    def __init__(self, variant=None):
        self.add_sums = functools.partial(dist_ref.add_sums, variant=variant, tile=4)
        self.key = functools.partial(dist_ref.diameter2_key, variant=variant) if variant == "past_end" else dist_ref.diameter2_key


def failed_checks(scorer):
    """Every check of this file on one scorer -> the names of those it fails."""
    failed = []

    def check(name, ok):
        if not ok:
            failed.append(name)

    vertices, est, gt = integer_case()
    for k in (0, 20, 30, -1):
        for symmetric in (False, True):
            sums, status = scorer.add_sums(vertices, est, gt, symmetric, k)
            check(f"exact sums, symmetric {symmetric}, k {k}", sums.tolist() == exact_sums(vertices, est, gt, symmetric, k) and not status.any())
    sums, _ = scorer.add_sums(vertices, est[:1], gt[:1], True, 20)
    check("est = gt scores ADD-S 0", sums.tolist() == [0])
    check("the diameter's square is the exact integer", scorer.key(vertices) == key_of(exact_diameter2(vertices)))
    check("one vertex has diameter 0", scorer.key(vertices[:1]) == 0)
    # a pure translation t: ADD = |t| for every vertex -- (3, 4, 12) has length 13
    moved = est.copy()
    moved[:, :3, 3] += (3, -4, 12)
    sums, _ = scorer.add_sums(vertices, moved, est, False, 20)
    check("a translation by t scores ADD |t|", sums.tolist() == [len(vertices) * 13 << 20] * len(est))
    # a set closed under a quarter turn, moved by that turn: ADD-S exactly 0, ADD > 0
    ring = closed_set()
    pose = rigid(quarter_turns()[7], (5, -3, 40))
    s_sym, _ = scorer.add_sums(ring, (pose @ TURN_Z)[None], pose[None], True, 20)
    s_add, _ = scorer.add_sums(ring, (pose @ TURN_Z)[None], pose[None], False, 20)
    check("a symmetric set moved by its symmetry scores ADD-S 0 and ADD > 0", s_sym.tolist() == [0] and s_add[0] > len(ring) << 20)
    # the direction: ground truth -> estimate
    for k in (0, 20):
        sums, _ = scorer.add_sums(DIRECTION_VERTICES, np.eye(4)[None], DIRECTION_GT[None], True, k)
        check(f"the direction is ground truth -> estimate, k {k}", sums.tolist() == [(2 << k) + (8 << k) + exact_q(5, k)])
    # the nearest point at index V - 1
    v6, e6, g6 = last_index_case()
    sums, _ = scorer.add_sums(v6, e6, g6, True, 20)
    check("the nearest point at the last index", sums.tolist() == exact_sums(v6, e6, g6, True, 20))
    return failed


def test_restatement_equals_exact_arithmetic_and_the_planted_cases():
    assert failed_checks(Scorer()) == []
    # the cases say what they claim
    vertices, est, gt = integer_case()
    adds, add = exact_sums(vertices, est, gt, True, 20), exact_sums(vertices, est, gt, False, 20)
    assert adds[0] == add[0] == 0 and all(a <= b for a, b in zip(adds, add)) and sum(a < b for a, b in zip(adds, add)) >= 7
    assert len(set(add)) == 10 and exact_diameter2(vertices) > 1000
    e, g = exact_points(np.eye(4), DIRECTION_VERTICES), exact_points(DIRECTION_GT, DIRECTION_VERTICES)
    assert sorted(min(exact_d2(gi, ej) for ej in e) for gi in g) == [4, 5, 64]           # ground truth -> estimate
    assert sorted(min(exact_d2(ei, gj) for gj in g) for ei in e) == [4, 64, 64]          # estimate -> ground truth: another number
    v6, e6, g6 = last_index_case()
    _, idx = dist_ref.nearest(dist_ref.transform(g6[0], v6), dist_ref.transform(e6[0], v6))
    assert idx.tolist() == [5] * 6
    ring = closed_set()
    assert len(ring) == 44 and len({tuple(p) for p in ring.tolist()}) == 44
    assert {tuple(p) for p in exact_points(TURN_Z, ring)} == {tuple(int(c) for c in p) for p in ring.tolist()}
    assert exact_q(2, 0) == 1 and exact_q(3, 0) == 2 and exact_q(6, 0) == 2 and exact_q(7, 0) == 3   # sqrt 1.41 1.73 2.45 2.65
    assert exact_q(9, -1) == 2 and exact_q(25, -1) == 2 and exact_q(1, -1) == 0          # 1.5 -> 2, 2.5 -> 2, 0.5 -> 0: half to even


@pytest.mark.parametrize("variant", list(dist_ref.VARIANTS) + ["past_end"])
def test_the_checks_reject_wrong_scorers(variant):
    """The reversed direction (estimate -> ground truth); a mean of squares (no root); a floor in place of rint; a minimum that
    skips j = i; an ADD-S that stops at a tile boundary (tiles of 4 here: the last, partial tile is never visited); a diameter
    over i <= j <= V that reads one vertex past the end (the origin stands for what lies there)."""
    failed = failed_checks(Scorer(variant))
    must = {"reversed": "the direction is ground truth -> estimate, k 20", "mean_of_squares": "a translation by t scores ADD |t|",
            "floor": "exact sums, symmetric False, k 0", "skip_self": "est = gt scores ADD-S 0", "tile_stop": "the nearest point at the last index",
            "past_end": "the diameter's square is the exact integer"}[variant]
    assert must in failed, failed


def test_restatement_status_bits():
    vertices, est, gt = integer_case()
    est, gt = est[:3].copy(), gt[:3].copy()
    base = [dist_ref.add_sums(vertices, est, gt, s, 20) for s in (False, True)]
    for s in (False, True):
        assert not base[s][1].any()
        e2 = est.copy()
        e2[1, 0, 3] = np.inf
        sums, status = dist_ref.add_sums(vertices, e2, gt, s, 20)
        assert status[1] & 1 and status[[0, 2]].tolist() == [0, 0] and sums[[0, 2]].tolist() == base[s][0][[0, 2]].tolist()
        g2 = gt.copy()
        g2[2, 1, 1] = np.nan
        sums, status = dist_ref.add_sums(vertices, est, g2, s, 20)
        assert status.tolist() == [0, 0, 3] and sums[:2].tolist() == base[s][0][:2].tolist()
        far = gt.copy()
        far[0, 2, 3] += 2.0 ** 23                                                    # 2^23 units = 2^43 quanta of 2^-20
        sums, status = dist_ref.add_sums(vertices, est, far, s, 20)
        assert status.tolist() == [2, 0, 0] and sums[1:].tolist() == base[s][0][1:].tolist()
        sums, status = dist_ref.add_sums(vertices, est, far, s, 0)                  # in range at k = 0
        assert status.tolist() == [0, 0, 0]
        vn = vertices.copy()
        vn[5, 2] = np.nan
        assert dist_ref.add_sums(vn, est, gt, s, 20)[1].tolist() == [3, 3, 3]
    assert np.isposinf(dist_ref.errors_from_sums([5, 6], [0, 2], 3, 20)[1])
    vn = vertices.copy()
    vn[7, 0] = np.inf
    assert dist_ref.diameter2_key(vn) == dist_ref.BAD_KEY and dist_ref.diameter2_key(vn[7:8]) == 0
    with pytest.raises(ValueError):
        dist_ref.diameter(vn)


# ---------------------------------------------------------------------------------------------- nearest neighbours against a KD-tree
def test_nearest_neighbours_against_a_kd_tree():
    """Random float vertices and poses: the restatement's nearest estimate point of every ground-truth point is the one scipy's
    cKDTree finds, up to exact ties (then the two candidates have the same d2, bit for bit)."""
    spatial = pytest.importorskip("scipy.spatial")
    from gigapose_testing import eval_cases as cases

    rs = np.random.RandomState(31)
    vertices = rs.uniform(-60, 60, (700, 3)).astype(np.float32)
    gt = cases.rigid(cases.rotation(rs), (10.0, -20.0, 600.0))
    est = gt @ cases.small_motion(rs, 0.3, 8.0)
    e, g = dist_ref.transform(est, vertices), dist_ref.transform(gt, vertices)
    vals, idx = dist_ref.nearest(g, e)
    _, tree_idx = spatial.cKDTree(e).query(g)
    assert (dist_ref.dist2(g, e[tree_idx]) == vals).all()
    assert (idx == tree_idx).mean() > 0.99 and (idx != np.arange(700)).sum() > 100   # and the nearest is often another vertex
    back, _ = dist_ref.nearest(e, g)
    assert (back != vals).sum() > 100                                                # the other direction: other numbers


# ---------------------------------------------------------------------------------------------- AddScorer over the restatement
def brute_force_matches(errors, threshold):
    taken = []
    for row in errors:
        best = None
        for g, err in enumerate(row):
            if g not in taken and (best is None or err < row[best]):
                best = g
        if best is not None and row[best] < threshold:
            taken.append(best)
    return len(taken)


def test_add_scorer_recalls_and_aucs_on_a_hand_case(monkeypatch):
    """AddScorer with the restatement standing in for the two GPU calls: object 1 (the closed set, listed as symmetric, no diameter
    given) and object 2 (asymmetric, diameter given), two images.  The recalls and AUCs are recomputed from the restatement's
    errors with the brute-force matcher, threshold by threshold."""
    from gigapose_testing import eval_cases as cases

    monkeypatch.setattr(distances, "add_errors", lambda v, est, gt, symmetric=False, k=20, device="cuda":
                        {"errors": torch.from_numpy(dist_ref.add_errors(v, est, gt, symmetric, k))})
    monkeypatch.setattr(distances, "model_diameter", lambda v, device="cuda": dist_ref.diameter(v))
    rs = np.random.RandomState(41)
    ring = closed_set() * np.float32(2.0)
    lump = rs.uniform(-40, 40, (50, 3)).astype(np.float32)
    models = {1: dict(vertices=ring, symmetries_discrete=[TURN_Z.reshape(-1).tolist()]), 2: dict(vertices=lump, diameter=dist_ref.diameter(lump))}
    poses = {key: [(obj, cases.rigid(cases.rotation(rs), t)) for obj, t in items] for key, items in
             {(3, 1): [(1, (-60.0, -30.0, 420.0)), (1, (50.0, 35.0, 380.0)), (2, (40.0, -45.0, 450.0))],
              (3, 2): [(2, (-30.0, 20.0, 400.0)), (1, (45.0, -10.0, 460.0))]}.items()}
    gts = {key: [dict(obj_id=o, cam_R_m2c=P[:3, :3].reshape(-1), cam_t_m2c=P[:3, 3]) for o, P in items] for key, items in poses.items()}
    targets = [dict(scene_id=3, im_id=1, obj_id=1, inst_count=2), dict(scene_id=3, im_id=1, obj_id=2, inst_count=1),
               dict(scene_id=3, im_id=2, obj_id=1, inst_count=1), dict(scene_id=3, im_id=2, obj_id=2, inst_count=1)]
    motions = [cases.small_motion(rs, 0.0, 0.0), TURN_Z, cases.small_motion(rs, 0.02, 3.0), cases.small_motion(rs, 0.3, 60.0),
               cases.small_motion(rs, 0.05, 3.0) @ TURN_Z]                           # exact, a symmetry, close, far, close up to the symmetry
    estimates, i = [], 0
    for key in sorted(poses):
        for obj, P in poses[key]:
            for h, extra in enumerate((np.eye(4), cases.small_motion(rs, 0.4, 30.0))):
                Q = P @ motions[i] @ extra
                estimates.append(dict(scene_id=key[0], im_id=key[1], obj_id=obj, score=0.9 - 0.1 * i - 0.3 * h, R=Q[:3, :3], t=Q[:3, 3]))
            i += 1
    scorer = distances.AddScorer(models, targets, gts, tau_max=50.0)
    got = scorer.score(estimates)
    assert scorer.diameters()[1] == dist_ref.diameter(ring) and scorer.symmetric == {1: True, 2: False}
    per = []
    for t, kept, g_list in evaluate.group_estimates(targets, gts, estimates):
        v = models[t["obj_id"]]["vertices"]
        E, G = len(kept), len(g_list)
        assert E == t["inst_count"]
        est = np.stack([cases.rigid(e["R"], e["t"]) for e in kept for _ in g_list])
        gt = np.stack([cases.rigid(np.reshape(g["cam_R_m2c"], (3, 3)), g["cam_t_m2c"]) for _ in kept for g in g_list])
        per.append((t["obj_id"], {s: dist_ref.add_errors(v, est, gt, s).reshape(E, G).tolist() for s in (False, True)}))
    diam = {1: dist_ref.diameter(ring), 2: models[2]["diameter"]}
    assert got["targets"] == 5
    for name, pick in (("add", lambda o: False), ("adds", lambda o: True), ("add_s", lambda o: o == 1)):
        assert got["recall_" + name] == sum(brute_force_matches(e[pick(o)], 0.1 * diam[o]) for o, e in per) / 5
        curve = [sum(brute_force_matches(e[pick(o)], 50.0 * j / 100) for o, e in per) / 5 for j in range(1, 101)]
        assert got["auc_" + name] == float(np.mean(curve))
    # what the motions must give: ADD misses the two estimates moved by the symmetry, ADD-S does not
    assert got["recall_add"] == 0.4 and got["recall_adds"] == 0.8 and got["recall_add_s"] == 0.8
    assert 0 < got["auc_add"] < got["auc_add_s"] <= got["auc_adds"] < 1
    exact = [dict(scene_id=key[0], im_id=key[1], obj_id=o, score=0.5, R=P[:3, :3], t=P[:3, 3]) for key in sorted(poses) for o, P in poses[key]]
    best = scorer.score(exact)
    assert best["recall_add"] == best["recall_adds"] == best["recall_add_s"] == 1.0
    assert best["auc_add"] == best["auc_adds"] == best["auc_add_s"] == 1.0 and best["targets"] == 5
    assert scorer.score([])["recall_add"] == 0.0
