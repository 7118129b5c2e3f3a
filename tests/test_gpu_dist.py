"""GPU: ADD, ADD-S and the model diameter (libgigapose_dist.so, gigapose_amd/distances.py).

gpd_add, gpd_adds and gpd_diameter2 against the numpy restatement (gigapose_testing/dist_ref.py, written from the header and held
to exact integer arithmetic by tests/test_dist_host.py) bit for bit -- sums, status words and the diameter's key -- at every size
where the kernels take another path (one lane, a thread's 4 points, a chunk of 1024 query points and its neighbours, one to three
staged tiles); the nearest point planted at the ends of the tiles; exact ties; the invariances an integer sum must have; the
bad-input rules; the limits (65535 pairs in one call, the chunking beyond); gpd_root against numpy.sqrt on the hard cases of
rounding; then model_diameter and AddScorer end to end."""
import functools
import math

import numpy as np
import pytest
import torch

from gigapose_testing import dist_ref, meshes
from gigapose_testing import eval_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (0, 20, 40)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} of {got.size} values differ"


def device_sums(vertices, est, gt, symmetric, k=20):
    from gigapose_amd import distances

    sums, status = distances.add_sums(_t(np.asarray(vertices, np.float32)), _t(np.asarray(est, np.float64)), _t(np.asarray(gt, np.float64)),
                                      symmetric, k)
    return sums.cpu().numpy(), status.cpu().numpy()


def device_key(vertices):
    from gigapose_amd import distances

    return int(distances.diameter2_key(_t(np.asarray(vertices, np.float32))).cpu().numpy().view(np.uint64)[0])


@functools.lru_cache(maxsize=None)
def master():
    """2049 random f32 vertices within +-60 and 7 pairs: ground-truth poses in front of a camera, estimates moved by a rotation
    of 0.01 rad and a shift below 0.5, so that ADD stays below 4 units = 2^42 quanta at k = 40.  Every (V, N) case is a prefix."""
    rs = np.random.RandomState(51)
    vertices = rs.uniform(-60, 60, (2049, 3)).astype(np.float32)
    gt = np.stack([cases.rigid(cases.rotation(rs), (rs.uniform(-80, 80), rs.uniform(-60, 60), rs.uniform(400, 900))) for _ in range(7)])
    est = np.stack([g @ cases.small_motion(rs, 0.01, 0.5) for g in gt])
    return vertices, est, gt


# ---------------------------------------------------------------------------------------------- 1. gpd_add / gpd_adds
@pytest.mark.parametrize("V", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_add_and_adds_equal_the_restatement(V):
    """V around a thread's first point (256), a workgroup's chunk and a staged tile (1024: V = 1025 needs a second workgroup, a
    second tile and the atomic merge), three tiles (2049); N = 1, 3, 7; k = 0, 20, 40.  One pass of the restatement per V and
    kernel serves every N and k."""
    vertices, est, gt = master()
    for symmetric in (False, True):
        want = dist_ref.add_sums(vertices[:V], est, gt, symmetric, KS)
        for k in KS:
            assert not want[k][1].any() and (k == 0 or (want[k][0] > 0).all()), (symmetric, k)
            for N in (1, 3, 7):
                sums, status = device_sums(vertices[:V], est[:N], gt[:N], symmetric, k)
                assert_bits(sums, want[k][0][:N], f"sums at V {V} N {N} k {k} symmetric {symmetric}")
                assert_bits(status, want[k][1][:N], f"status at V {V} N {N} k {k} symmetric {symmetric}")
    if V >= 255:
        add, adds = dist_ref.add_sums(vertices[:V], est, gt, False, 20)[0], dist_ref.add_sums(vertices[:V], est, gt, True, 20)[0]
        assert (adds <= add).all() and len(set(add.tolist())) == 7


@pytest.mark.parametrize("where", [0, 1023, 1024, 2048])
def test_planted_nearest_point(where):
    """2049 vertices within +-5 of the origin and ONE at (103, 1, 1), at the first slot of the first tile, on both sides of the
    first tile boundary, and at the last vertex of the last (one-slot) tile.  The ground truth is shifted by (100, 0, 0), so the
    nearest estimate point of EVERY ground-truth point is the planted one: a kernel that misses that slot is off by ~90 per vertex."""
    rs = np.random.RandomState(where)
    vertices = rs.uniform(-5, 5, (2049, 3)).astype(np.float32)
    vertices[where] = (103.0, 1.0, 1.0)
    est = cases.small_motion(rs, 0.002, 0.1)[None]
    gt = (est[0] @ cases.rigid(np.eye(3), (100.0, 0.0, 0.0)))[None]
    _, idx = dist_ref.nearest(dist_ref.transform(gt[0], vertices), dist_ref.transform(est[0], vertices))
    assert (idx == where).all()
    for k in (0, 20):
        want = dist_ref.add_sums(vertices, est, gt, True, k)
        got = device_sums(vertices, est, gt, True, k)
        assert_bits(got[0], want[0], f"sums, k {k}")
        assert_bits(got[1], want[1], f"status, k {k}")
    assert want[0][0] < 2049 * 12 << 20                                              # ~ 4 .. 11 per vertex, not ~ 95


def test_exact_ties_and_the_direction():
    """Vertices on the integer lattice within +-3 (many coincide), the ground truth shifted by half a cell in x and y: every
    ground-truth point is equally far from two or four estimate points, every d2 is exact.  Then the two directions of ADD-S on a
    case where they differ: the kernel takes ground truth -> estimate."""
    rs = np.random.RandomState(5)
    vertices = rs.randint(-3, 4, (1300, 3)).astype(np.float32)
    est, gt = np.eye(4)[None], cases.rigid(np.eye(3), (0.5, 0.5, 0.0))[None]
    for k in (0, 20):
        want = dist_ref.add_sums(vertices, est, gt, True, k)
        got = device_sums(vertices, est, gt, True, k)
        assert_bits(got[0], want[0], f"sums, k {k}")
        assert_bits(got[1], want[1], f"status, k {k}")
    v3 = np.asarray([(0, 0, 0), (10, 0, 0), (0, 1, 0)], np.float32)
    shift = cases.rigid(np.eye(3), (8.0, 0.0, 0.0))[None]
    sums, _ = device_sums(v3, np.eye(4)[None], shift, True, 20)
    assert sums.tolist() == [(10 << 20) + int(np.rint(np.sqrt(5.0) * 2 ** 20))]      # 2 + 8 + sqrt(5); the other direction: 18
    sums, _ = device_sums(v3, shift, np.eye(4)[None], True, 20)                      # the roles exchanged
    assert sums.tolist() == [18 << 20]


def test_results_do_not_depend_on_order():
    """Permuted vertices leave every sum; permuted pairs permute them; a second run gives the same bits."""
    vertices, est, gt = master()
    vertices = vertices[:1500]
    rs = np.random.RandomState(2)
    pv, pn = rs.permutation(len(vertices)), rs.permutation(7)
    for symmetric in (False, True):
        base = device_sums(vertices, est, gt, symmetric)
        again = device_sums(vertices, est, gt, symmetric)
        by_v = device_sums(vertices[pv], est, gt, symmetric)
        by_n = device_sums(vertices, est[pn], gt[pn], symmetric)
        for c, name in enumerate(("sums", "status")):
            assert_bits(again[c], base[c], f"{name}, second run")
            assert_bits(by_v[c], base[c], f"{name}, permuted vertices")
            assert_bits(by_n[c], base[c][pn], f"{name}, permuted pairs")
        assert len(set(base[0].tolist())) == 7


def test_bad_inputs_set_the_status_of_that_pair_only():
    vertices, est, gt = master()
    vertices, est, gt = vertices[:1100], est[:3], gt[:3]
    for symmetric in (False, True):
        base = device_sums(vertices, est, gt, symmetric)
        assert base[1].tolist() == [0, 0, 0]
        e2 = est.copy()
        e2[1, 0, 3] = np.inf                                                         # an infinite translation: pair 1 only
        for e_, g_ in ((e2, gt), (est, np.where(np.isinf(e2), np.inf, gt))):         #   ... on the estimate's side, on the ground truth's
            sums, status = device_sums(vertices, e_, g_, symmetric)
            assert_bits(status, dist_ref.add_sums(vertices, e_, g_, symmetric)[1], "status")
            assert status[1] & 1 and status[[0, 2]].tolist() == [0, 0]
            assert_bits(sums[[0, 2]], base[0][[0, 2]], "sums of the other pairs")
        far = gt.copy()
        far[2, 0, 3] += 2.0 ** 23                                                    # 2^23 units are 2^43 quanta at k = 20: out of range
        sums, status = device_sums(vertices, est, far, symmetric)
        assert status.tolist() == [0, 0, 2] and dist_ref.add_sums(vertices, est, far, symmetric)[1].tolist() == [0, 0, 2]
        assert_bits(sums[:2], base[0][:2], "sums of the other pairs")
        sums, status = device_sums(vertices, est, far, symmetric, k=0)               # ... and in range at k = 0
        assert status.tolist() == [0, 0, 0]
        assert_bits(sums, dist_ref.add_sums(vertices, est, far, symmetric, 0)[0], "sums at k = 0")
        vn = vertices.copy()
        vn[1050, 2] = np.nan                                                         # a NaN vertex belongs to every pair
        sums, status = device_sums(vn, est, gt, symmetric)
        assert status.tolist() == [3, 3, 3] and dist_ref.add_sums(vn, est, gt, symmetric)[1].tolist() == [3, 3, 3]


def test_65535_pairs_in_one_call_and_the_chunking_beyond():
    """V = 2: 65535 pairs are one launch (the grid's second dimension); add_errors splits 65537 into two."""
    from gigapose_amd import distances

    N = 65537
    rs = np.random.RandomState(8)
    vertices = np.asarray([[3.0, -2.0, 1.0], [-1.5, 4.0, 2.0]], np.float32)
    est, gt = np.tile(np.eye(4), (N, 1, 1)), np.tile(np.eye(4), (N, 1, 1))
    est[:, :3, 3] = rs.uniform(-50, 50, (N, 3)) + (0, 0, 500)
    gt[:, :3, 3] = rs.uniform(-50, 50, (N, 3)) + (0, 0, 500)
    gt[:, :3, :3] = cases.rotation(rs)
    for symmetric in (False, True):
        want = dist_ref.add_sums(vertices, est, gt, symmetric)
        got = device_sums(vertices, est[:65535], gt[:65535], symmetric)
        assert_bits(got[0], want[0][:65535], "sums of 65535 pairs")
        assert_bits(got[1], want[1][:65535], "status of 65535 pairs")
        with pytest.raises(ValueError, match="65535"):
            device_sums(vertices, est[:65536], gt[:65536], symmetric)
        out = distances.add_errors(vertices, est, gt, symmetric)
        assert out["errors"].dtype == torch.float64 and not out["errors"].is_cuda and out["errors"].shape == (N,)
        assert_bits(out["errors"].numpy(), dist_ref.errors_from_sums(want[0], want[1], 2, 20), "errors of 65537 pairs")
        assert not out["status"].any() and len(set(out["errors"].numpy()[[0, 65534, 65535, 65536]].tolist())) == 4


def test_add_errors_reports_infinity_where_a_status_bit_is_set():
    from gigapose_amd import distances

    vertices, est, gt = master()
    e2 = est[:3].copy()
    e2[1, 2, 3] = np.nan
    out = distances.add_errors(torch.from_numpy(vertices[:300]), e2, torch.from_numpy(gt[:3]), symmetric=True)
    want = dist_ref.add_sums(vertices[:300], e2, gt[:3], True)
    assert_bits(out["errors"].numpy(), dist_ref.errors_from_sums(want[0], want[1], 300, 20), "errors")
    assert np.isposinf(out["errors"].numpy()[1]) and out["status"].tolist() == [0, 3, 0] and np.isfinite(out["errors"].numpy()[[0, 2]]).all()
    assert abs(out["errors"].numpy()[0] - np.sqrt(dist_ref.nearest(dist_ref.transform(gt[0], vertices[:300]),
                                                                    dist_ref.transform(e2[0], vertices[:300]))[0]).mean()) < 1e-5


# ---------------------------------------------------------------------------------------------- 2. gpd_root
def device_roots(x):
    from gigapose_amd import distances

    return distances.roots(_t(np.asarray(x, np.float64))).cpu().numpy()


def test_root_is_the_correctly_rounded_square_root():
    """Perfect squares and their two neighbours; the ends of the normal range, subnormals, 0 and +inf; 1e5 random doubles over
    the whole exponent range; and the hard cases of rounding: for 5000 random 53-bit M and exponents e, the two doubles next to
    the square of the midpoint (M + 1/2) * 2^e, built with Python integers -- the root of the lower one rounds to M * 2^e, the
    root of the upper one to (M + 1) * 2^e, by a margin of about 2^-54 of a unit in the last place."""
    rs = np.random.RandomState(13)
    a = rs.randint(1, 2 ** 26, 3000).astype(np.float64)
    sq = a * a
    parts = [sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)]
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    parts.append(np.asarray([0.0, np.inf, tiny, np.nextafter(tiny, 1.0), np.nextafter(tiny, 0.0), big, np.nextafter(big, 0.0), 5e-324, 1e-320,
                             3e-310, 2.0 ** -500, np.nextafter(2.0 ** -500, 0.0), 1.0, 2.0, 4.0, np.nextafter(1.0, 0.0), np.nextafter(4.0, 0.0)]))
    bits = rs.randint(0, 2 ** 63 - 1, 100000, dtype=np.int64)
    rnd = bits.view(np.float64)
    parts.append(rnd[np.isfinite(rnd)])
    parts.append(rs.randint(1, 2 ** 52, 2000, dtype=np.int64).view(np.float64))        # subnormals
    hard, expect = [], []
    for _ in range(5000):
        M, e = int(rs.randint(2 ** 52, 2 ** 53, dtype=np.int64)), int(rs.randint(-300, 300))
        S = (2 * M + 1) ** 2                                                         # the square of the midpoint, times 4 * 2^-2e: odd
        shift = S.bit_length() - 53
        lo = S >> shift                                                              # the 53 leading bits: the double just below
        hard += [math.ldexp(lo, shift + 2 * e - 2), math.ldexp(lo + 1, shift + 2 * e - 2)]
        expect += [math.ldexp(M, e), math.ldexp(M + 1, e)]
    hard, expect = np.asarray(hard), np.asarray(expect)
    assert (np.sqrt(hard) == expect).all() and len(hard) == 10000                    # numpy rounds them as the integers say
    parts.append(hard)
    x = np.concatenate(parts)
    got = device_roots(x)
    want = np.sqrt(x)
    assert_bits(got, want, "root")
    assert_bits(device_roots(np.asarray([-0.0, -1.0, np.nan]))[:1], np.asarray([-0.0]), "root of -0")
    assert np.isnan(device_roots(np.asarray([-1.0, np.nan, -np.inf]))).all()


# ---------------------------------------------------------------------------------------------- 3. the diameter
@pytest.mark.parametrize("V", [1, 2, 3, 257, 1024, 1025, 2049])
def test_diameter_key_equals_the_restatement(V):
    """One vertex (no pair: 0); one workgroup on the diagonal; V = 1025 and 2049: 3 and 6 tiles of the upper triangle merged by
    the atomic maximum.  Then the two farthest vertices planted in the last tile's last slot and the first tile's first slot."""
    vertices, _, _ = master()
    want = dist_ref.diameter2_key(vertices[:V])
    assert device_key(vertices[:V]) == want and (want > 0) == (V > 1)
    if V >= 257:
        v = vertices[:V].copy()
        v[0], v[V - 1] = (-200.0, 50.0, 7.0), (300.0, -20.0, 11.0)
        assert device_key(v) == dist_ref.diameter2_key(v) == int(np.asarray([500.0 ** 2 + 70.0 ** 2 + 4.0 ** 2]).view(np.uint64)[0])
        v[V // 2, 1] = np.inf
        assert device_key(v) == dist_ref.diameter2_key(v) == dist_ref.BAD_KEY
    else:
        v = vertices[:V].copy()
        v[0, 0] = np.nan
        assert device_key(v) == dist_ref.diameter2_key(v) == (dist_ref.BAD_KEY if V > 1 else 0)


def test_model_diameter():
    from gigapose_amd import distances

    box = meshes.box((60.0, 40.0, 30.0))[0]                                          # 24 vertices on 8 corners: 60^2 + 40^2 + 30^2 = 6100
    assert distances.model_diameter(box) == np.sqrt(6100.0)
    assert distances.model_diameter(torch.from_numpy(box).to(DEV)) == np.sqrt(6100.0)
    vertices, _, _ = master()
    assert distances.model_diameter(vertices[:1]) == 0.0
    d = distances.model_diameter(vertices[:1025])
    assert d == dist_ref.diameter(vertices[:1025]) and isinstance(d, float)
    v64 = vertices[:1025].astype(np.float64)
    assert abs(d - np.sqrt(((v64[:, None] - v64[None]) ** 2).sum(axis=2).max())) < 1e-9
    for bad in (np.nan, np.inf):
        v = vertices[:300].copy()
        v[299, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            distances.model_diameter(v)
        with pytest.raises(ValueError, match="not finite"):
            distances.model_diameter(v[299:])


# ---------------------------------------------------------------------------------------------- 4. AddScorer over a csv
BOX_SIZE = (60.0, 40.0, 30.0)
BOX_INFO = {"symmetries_discrete": [cases.HALF_TURN_X, cases.HALF_TURN_Y, cases.HALF_TURN_Z]}


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


def scorer_scene():
    """Two objects (1: an icosphere squeezed to a box-like ellipsoid with the three half turns listed, no diameter given;
    2: the asymmetric three_boxes, diameter given), two images of scene 2."""
    rs = np.random.RandomState(15)
    ball = (meshes.icosphere(2, 1.0)[0] * np.asarray(BOX_SIZE, np.float32) / 2).astype(np.float32)
    lump = meshes.three_boxes(30.0)[0]
    models = {1: dict(vertices=ball, **BOX_INFO), 2: dict(vertices=lump, diameter=dist_ref.diameter(lump))}
    layout = {(2, 1): [(1, (-60.0, -30.0, 420.0)), (1, (50.0, 35.0, 380.0)), (2, (40.0, -45.0, 450.0))],
              (2, 2): [(2, (-30.0, 20.0, 400.0)), (1, (45.0, -10.0, 460.0))]}
    gts = {}
    for key, items in layout.items():
        gts[key] = []
        for obj, t in items:
            P = cases.rigid(cases.rotation(rs), t).astype(np.float32).astype(np.float64)
            gts[key].append(dict(obj_id=obj, cam_R_m2c=P[:3, :3].reshape(-1).tolist(), cam_t_m2c=P[:3, 3].tolist(), pose=P))
    targets = [dict(scene_id=2, im_id=1, obj_id=1, inst_count=2), dict(scene_id=2, im_id=1, obj_id=2, inst_count=1),
               dict(scene_id=2, im_id=2, obj_id=1, inst_count=1), dict(scene_id=2, im_id=2, obj_id=2, inst_count=1)]
    return models, targets, gts


def write_csv(tmp_path, name, gts, perturb, k=2):
    """One detection per ground truth, k hypotheses each, in the npz layout GigaPose.filter_and_save writes, merged by
    inout.save_predictions_from_batched_predictions.  -> the MultiHypothesis csv."""
    from gigapose_amd import inout

    out_dir = tmp_path / name
    out_dir.mkdir()
    rows = [(key, g) for key in sorted(gts) for g in gts[key]]
    for b, part in enumerate((rows[:3], rows[3:])):
        n = len(part)
        poses, scores = np.zeros((n, k, 4, 4), np.float32), np.zeros((n, k), np.float32)
        for i, (key, g) in enumerate(part):
            for h in range(k):
                poses[i, h], scores[i, h] = perturb(b * 3 + i, h, g)
        np.savez(str(out_dir / f"{b}.npz"), scene_id=np.asarray([key[0] for key, _ in part], np.int32),
                 im_id=np.asarray([key[1] for key, _ in part], np.int32), object_id=np.asarray([g["obj_id"] for _, g in part], np.int32),
                 time=np.full(n, 0.05), detection_time=np.full(n, 0.1), poses=poses, scores=scores)
    paths = inout.save_predictions_from_batched_predictions(str(out_dir), "tless", "gigapose", "run", is_refined=False)
    assert paths[1].endswith("MultiHypothesis.csv")
    return paths[1]


def test_add_scorer_over_a_csv(tmp_path):
    """Known perturbations: detection 0 exact, 1 moved by a half turn (a symmetry of the ellipsoid's vertex set: ADD-S ~ 0, ADD
    large), 2 shifted by 2 mm, 3 shifted by 25 mm -- its exact second hypothesis scores lower and is not kept --, 4 rotated by
    0.5 rad.  The recalls and AUCs equal those computed from the restatement's errors through the brute-force matcher."""
    from gigapose_amd import distances, evaluate

    models, targets, gts = scorer_scene()
    rs = np.random.RandomState(33)
    half_turn = np.asarray(cases.HALF_TURN_Z, np.float64).reshape(4, 4)

    def perturb(i, h, g):
        P = g["pose"].copy()
        if i == 1:
            P = P @ half_turn
        elif i == 2:
            P[:3, 3] += (2.0, 0.0, 0.0)
        elif i == 3 and h == 0:
            P[:3, 3] += (0.0, 25.0, 0.0)
        elif i == 4:
            P = P @ cases.small_motion(rs, 0.5, 0.0)
        if h == 1 and i != 3:
            P = P @ cases.small_motion(rs, 0.2, 8.0)
        return P.astype(np.float32), np.float32(0.9 - 0.1 * i - 0.3 * h)

    path = write_csv(tmp_path, "perturbed", gts, perturb)
    scorer = distances.AddScorer(models, targets, gts)
    got = scorer.score_csv(path)
    estimates = evaluate.read_estimates(path)
    assert len(estimates) == 10
    diam = {1: dist_ref.diameter(models[1]["vertices"]), 2: models[2]["diameter"]}
    assert scorer.diameters() == diam and abs(diam[1] - 60.0) < 1e-4                # the ellipsoid's long axis; it was computed on the GPU
    per = []
    for t, kept, g_list in scorer.pairs(estimates):
        v = models[t["obj_id"]]["vertices"]
        E, G = len(kept), len(g_list)
        assert E == t["inst_count"]
        est = np.stack([cases.rigid(e["R"], e["t"]) for e in kept for _ in g_list])
        gt = np.stack([g["pose"] for _ in kept for g in g_list])
        per.append((t["obj_id"], {s: dist_ref.errors_from_sums(*dist_ref.add_sums(v, est, gt, s), len(v), 20).reshape(E, G).tolist()
                                  for s in (False, True)}))
    assert got["targets"] == 5
    for name, pick in (("add", lambda o: False), ("adds", lambda o: True), ("add_s", lambda o: o == 1)):
        assert got["recall_" + name] == sum(brute_force_matches(e[pick(o)], 0.1 * diam[o]) for o, e in per) / 5, name
        curve = [sum(brute_force_matches(e[pick(o)], 100.0 * j / 100) for o, e in per) / 5 for j in range(1, 101)]
        assert got["auc_" + name] == float(np.mean(curve)), name
    # what the perturbations must give (thresholds: 6 mm for the ellipsoid, 5.9 mm for three_boxes): ADD accepts the exact
    # estimate and the one 2 mm off; ADD-S also the half-turned ellipsoid (0 to rounding) and the one rotated by 0.5 rad, whose
    # surface stays within ~3.6 mm of itself (ADD: 9.4 mm); the 25 mm shift fails both (ADD-S 17 mm); the mixed recall takes
    # ADD-S for the ellipsoid and ADD for three_boxes
    assert got["recall_add"] == 0.4 and got["recall_adds"] == 0.8 and got["recall_add_s"] == 0.8
    assert 0.5 < got["auc_add"] < got["auc_add_s"] <= got["auc_adds"] < 1.0
    exact = scorer.score_csv(write_csv(tmp_path, "exact", gts, lambda i, h, g: (g["pose"].astype(np.float32), np.float32(0.9 - 0.1 * i - 0.3 * h)), k=1))
    assert exact["recall_add"] == exact["recall_adds"] == exact["recall_add_s"] == 1.0
    assert exact["auc_add"] == exact["auc_adds"] == exact["auc_add_s"] == 1.0 and exact["targets"] == 5
