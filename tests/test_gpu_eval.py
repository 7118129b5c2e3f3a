"""GPU: scoring pose estimates (libgigapose_eval.so, gigapose_amd/evaluate.py).

gpe_mssd_mspd and gpe_vsd_counts against the numpy restatement (gigapose_testing/eval_ref.py, written from the header and held
to exact arithmetic by tests/test_eval_host.py) bit for bit, at every size where the kernels take another path (one lane, a
wave and its neighbours, a workgroup and its neighbours, several workgroups merging through the atomics; 1 to 630 symmetries);
the invariances an integer reduction must have; the bad-input rules; the limits (65535 pairs in one call, the chunking beyond,
an element offset past 2^31); then vsd_errors and PoseScorer end to end on procedural meshes drawn by MeshRenderer."""
import numpy as np
import pytest
import torch

from gigapose_testing import eval_cases as cases
from gigapose_testing import eval_ref, meshes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} of {got.size} values differ"


def device_errors(vertices, syms, est, gt, K, zmin=0.0):
    from gigapose_amd import evaluate

    d2, p2 = evaluate.mssd_mspd(_t(np.asarray(vertices, np.float32)), _t(np.asarray(syms, np.float64)), _t(est), _t(gt),
                                _t(np.asarray(K, np.float64).reshape(len(est), 9)), zmin)
    return d2.cpu().numpy(), p2.cpu().numpy()


@pytest.fixture(scope="module")
def cylinder_syms():
    from gigapose_amd import evaluate

    s = evaluate.symmetry_transforms(cases.CYLINDER)
    assert s.shape == (630, 4, 4)
    return s


@pytest.fixture(scope="module")
def master(cylinder_syms):
    """1025 vertices, 3 pairs: every (V, S, N) case below is a prefix of it."""
    return cases.pose_case(21, 1025, 3, cylinder_syms)


# ---------------------------------------------------------------------------------------------- 1. gpe_mssd_mspd
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_mssd_mspd_equals_the_restatement(master, cylinder_syms, V, N):
    """V around a wave (64), a workgroup's first pass (256) and its whole span (1024: V = 1025 needs a second workgroup and the
    atomic merge); S = 1, 2, 3, 65 (past one wave of the finish kernel), 630."""
    vertices, est, gt, K = master
    for S in (1, 2, 3, 65, 630):
        want_d, want_p = eval_ref.mssd_mspd2(vertices[:V], cylinder_syms[:S], est[:N], gt[:N], K[:N])
        assert np.isfinite(want_d).all() and np.isfinite(want_p).all() and (want_d > 0).all()
        got_d, got_p = device_errors(vertices[:V], cylinder_syms[:S], est[:N], gt[:N], K[:N])
        assert_bits(got_d, want_d, f"mssd2 at V {V} S {S} N {N}")
        assert_bits(got_p, want_p, f"mspd2 at V {V} S {S} N {N}")


@pytest.mark.parametrize("V", [300, 2500])
@pytest.mark.parametrize("where", ["first", "mid-wave", "last"])
def test_planted_maximum_and_minimum(cylinder_syms, V, where):
    """One vertex far from the others carries the maximum: planted at the first, a mid-wave and the last index (V = 2500: the
    last workgroup holds 452 vertices and repeats the last one in its idle lanes).  The estimate is the ground truth moved by the
    first / the last symmetry and a rotation of 0.004 rad, so the minimum sits there and its maximum at the far vertex."""
    syms = cylinder_syms[:65]
    index = {"first": 0, "mid-wave": 64 * 2 + 37, "last": V - 1}[where]
    rs = np.random.RandomState(V)
    vertices = rs.uniform(-5, 5, (V, 3)).astype(np.float32)
    vertices[index] = (70.0, -40.0, 55.0)
    gt = np.stack([cases.rigid(cases.rotation(rs), (10.0, -20.0, 600.0))] * 2)
    est = np.stack([gt[0] @ syms[0] @ cases.small_motion(rs, 0.004, 0.0), gt[1] @ syms[64] @ cases.small_motion(rs, 0.004, 0.0)])
    K = np.tile(cases.K_CAMERA, (2, 1))
    d2, p2, _, _ = eval_ref.deviations(vertices, syms, est, gt, K)
    for dev in (d2, p2):                                                             # the restatement finds both where planted
        assert dev.max(axis=2).argmin(axis=1).tolist() == [0, 64]
        assert dev[0, 0].argmax() == index and dev[1, 64].argmax() == index
    want_d, want_p = eval_ref.mssd_mspd2(vertices, syms, est, gt, K)
    got_d, got_p = device_errors(vertices, syms, est, gt, K)
    assert_bits(got_d, want_d, "mssd2")
    assert_bits(got_p, want_p, "mspd2")


def test_results_do_not_depend_on_order(master, cylinder_syms):
    """Permuted vertices and permuted symmetries (the identity kept first) leave every bit; permuted pairs permute the outputs;
    a second run gives the same bits."""
    vertices, est, gt, K = master
    syms = cylinder_syms[:65]
    rs = np.random.RandomState(2)
    base = device_errors(vertices, syms, est, gt, K)
    again = device_errors(vertices, syms, est, gt, K)
    pv = rs.permutation(len(vertices))
    ps = np.concatenate([[0], 1 + rs.permutation(len(syms) - 1)])
    pn = np.asarray([2, 0, 1])
    by_v = device_errors(vertices[pv], syms, est, gt, K)
    by_s = device_errors(vertices, syms[ps], est, gt, K)
    by_n = device_errors(vertices, syms, est[pn], gt[pn], K[pn])
    for c, name in enumerate(("mssd2", "mspd2")):
        assert_bits(again[c], base[c], f"{name}, second run")
        assert_bits(by_v[c], base[c], f"{name}, permuted vertices")
        assert_bits(by_s[c], base[c], f"{name}, permuted symmetries")
        assert_bits(by_n[c], base[c][pn], f"{name}, permuted pairs")
    assert len(set(base[0].tolist())) == 3


def test_bad_inputs_give_infinity_for_that_pair_only(master, cylinder_syms):
    vertices, est, gt, K = master
    vertices, syms = vertices[:300], cylinder_syms[:3]
    base_d, base_p = device_errors(vertices, syms, est, gt, K)
    others = [0, 2]
    e2 = est.copy()
    e2[1, 1, 2] = np.inf                                                             # an infinite pose entry: pair 1 only
    for e_, g_ in ((e2, gt), (est, np.where(np.isinf(e2), np.inf, gt))):             #   ... on the estimate's side, on the ground truth's
        d2, p2 = device_errors(vertices, syms, e_, g_, K)
        assert_bits(d2, eval_ref.mssd_mspd2(vertices, syms, e_, g_, K)[0], "mssd2")
        assert np.isposinf(d2[1]) and np.isposinf(p2[1])
        assert_bits(d2[others], base_d[others], "mssd2 of the other pairs")
        assert_bits(p2[others], base_p[others], "mspd2 of the other pairs")
    e3 = est.copy()
    e3[0, 1, 3] = np.nan                                                             # a NaN wins every comparison
    d2, p2 = device_errors(vertices, syms, e3, gt, K)
    assert np.isposinf(d2[0]) and np.isposinf(p2[0])
    assert_bits(d2[1:], base_d[1:], "mssd2 of the other pairs")
    vn = vertices.copy()
    vn[137, 2] = np.nan                                                              # a NaN vertex belongs to every pair
    d2, p2 = device_errors(vn, syms, est, gt, K)
    assert np.isposinf(d2).all() and np.isposinf(p2).all()
    # a vertex below zmin on one side only -- the nearest pair is pulled 30 closer on the estimate's side, then on the ground
    # truth's, and zmin put 15 behind its nearest vertex: mspd2 = +inf for that pair, nothing else changes
    dev = eval_ref.deviations(vertices, syms, est, gt, K)
    near = int(np.minimum(dev[2].min(axis=(1, 2)), dev[3].min(axis=(1, 2))).argmin())
    for side in (0, 1):
        e_, g_ = est.copy(), gt.copy()
        (e_, g_)[side][near, 2, 3] -= 30.0
        dev = eval_ref.deviations(vertices, syms, e_, g_, K)
        z = [dev[2].min(axis=(1, 2)), dev[3].min(axis=(1, 2))]
        zmin = z[side][near] + 15.0
        assert z[1 - side][near] > zmin + 5 and np.delete(np.minimum(z[0], z[1]), near).min() > zmin + 5
        want_d, want_p = eval_ref.mssd_mspd2(vertices, syms, e_, g_, K, zmin=zmin)
        free_d, free_p = eval_ref.mssd_mspd2(vertices, syms, e_, g_, K, zmin=0.0)
        assert np.isposinf(want_p[near]) and np.isfinite(free_p).all() and (np.delete(want_p, near) == np.delete(free_p, near)).all()
        d2, p2 = device_errors(vertices, syms, e_, g_, K, zmin=zmin)
        assert_bits(d2, free_d, "mssd2 under zmin")
        assert_bits(p2, want_p, "mspd2 under zmin")
    far = device_errors(vertices, syms, est, gt, K, zmin=-1e300)
    assert_bits(far[1], base_p, "mspd2 with zmin far behind the camera")


def test_65535_pairs_in_one_call_and_the_chunking_beyond():
    """V = S = 1: 65535 pairs are one launch (the grid's second dimension); pose_errors splits 65537 into two."""
    from gigapose_amd import evaluate

    N = 65537
    rs = np.random.RandomState(8)
    vertices, syms = np.asarray([[3.0, -2.0, 1.0]], np.float32), np.eye(4)[None]
    est, gt = np.tile(np.eye(4), (N, 1, 1)), np.tile(np.eye(4), (N, 1, 1))
    est[:, :3, 3] = rs.uniform(-50, 50, (N, 3)) + (0, 0, 500)
    gt[:, :3, 3] = rs.uniform(-50, 50, (N, 3)) + (0, 0, 500)
    K = np.tile(cases.K_CAMERA, (N, 1))
    want_d, want_p = eval_ref.mssd_mspd2(vertices, syms, est, gt, K)
    got_d, got_p = device_errors(vertices, syms, est[:65535], gt[:65535], K[:65535])
    assert_bits(got_d, want_d[:65535], "mssd2 of 65535 pairs")
    assert_bits(got_p, want_p[:65535], "mspd2 of 65535 pairs")
    with pytest.raises(ValueError, match="65535"):
        device_errors(vertices, syms, est[:65536], gt[:65536], K[:65536])
    mssd, mspd = evaluate.pose_errors(vertices, syms, est, gt, K)
    assert mssd.dtype == torch.float64 and not mssd.is_cuda and mssd.shape == (N,)
    assert_bits(mssd.numpy(), np.sqrt(want_d), "mssd of 65537 pairs")
    assert_bits(mspd.numpy(), np.sqrt(want_p), "mspd of 65537 pairs")
    assert len(set(mssd.numpy()[[0, 65534, 65535, 65536]].tolist())) == 4


# ---------------------------------------------------------------------------------------------- 2. gpe_vsd_counts
def random_maps(seed, N, H, W, T):
    """Depths on a grid of 1/4 with holes, negative, NaN and infinite pixels; rays on a grid of 1/64; thresholds on a grid of 1/8:
    comparisons fall on their boundary often.  M = 2 frames, R = 2 ray maps, mixed indices."""
    rs = np.random.RandomState(seed)

    def depth(n, base):
        d = (base + rs.randint(0, 17, (n, H, W)) / 4.0).astype(np.float32)
        d[rs.rand(n, H, W) < 0.3] = 0.0
        odd = rs.rand(n, H, W)
        d[odd < 0.02] = -1.5
        d[(odd >= 0.02) & (odd < 0.04)] = np.nan
        d[(odd >= 0.04) & (odd < 0.05)] = np.inf
        return d

    de, dg, dt = depth(N, 8.0), depth(N, 8.0), depth(2, 9.0)
    ray = 1.0 + rs.randint(0, 17, (2, H, W)) / 64.0
    frame, ray_index = rs.randint(0, 2, N).astype(np.int32), rs.randint(0, 2, N).astype(np.int32)
    if N >= 4:
        frame[:4], ray_index[:4] = [0, 1, 0, 1], [0, 0, 1, 1]
    thr = rs.randint(0, 25, (N, T)) / 8.0
    return de, dg, dt, frame, ray, ray_index, 1.0, thr


def device_counts(de, dg, dt, frame, ray, ray_index, delta, thr):
    from gigapose_amd import evaluate

    return evaluate.vsd_counts(_t(de), _t(dg), _t(dt), frame, _t(ray), ray_index, delta, _t(thr)).cpu().numpy()


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 33), (64, 64)])
def test_vsd_counts_equal_the_restatement(H, W, N):
    """One pixel; fewer than a wave; a part of one workgroup's 2048 pixels; two workgroups adding into the same counters."""
    for T in (1, 10, 16):
        args = random_maps(1000 * H + 10 * N + T, N, H, W, T)
        want = eval_ref.vsd_counts(*args)
        got = device_counts(*args)
        assert got.dtype == np.int64 and got.shape == (N, 2 + T)
        np.testing.assert_array_equal(got, want, err_msg=f"{H} x {W}, N {N}, T {T}")
        if H * W >= 500:
            assert (want[:, 0] > want[:, 1]).all() and (want[:, 1] > 0).all() and want[:, 2:].max() > 0
    np.testing.assert_array_equal(device_counts(*args), got)                        # a second run


def test_vsd_counts_at_480_x_640():
    args = random_maps(77, 4, 480, 640, 10)
    want = eval_ref.vsd_counts(*args)
    np.testing.assert_array_equal(device_counts(*args), want)
    assert want[:, 0].min() > 150000 and len({tuple(r) for r in want.tolist()}) == 4


def test_vsd_planted_cases():
    """The hand-built maps of the CPU suite (dyadic values: Dm - Dt exactly delta, a cost exactly on a threshold, holes, a fully
    occluded estimate, nothing visible, negative / NaN / infinite pixels), all in one call: the kernel against the set-based reading
    in exact arithmetic, not only against the restatement."""
    maps, ray, delta, thr = cases.vsd_cases()
    de, dg = np.stack([m[1] for m in maps]), np.stack([m[2] for m in maps])
    dt = np.stack([m[3] for m in maps])
    N = len(maps)
    got = device_counts(de, dg, dt, np.arange(N), ray[None], np.zeros(N, int), delta, np.tile(thr, (N, 1)))
    for n, (name, e, g, t) in enumerate(maps):
        assert got[n].tolist() == cases.vsd_by_sets(e, g, t, ray, delta, thr), name
    np.testing.assert_array_equal(got, eval_ref.vsd_counts(de, dg, dt, np.arange(N), ray[None], np.zeros(N, int), delta, np.tile(thr, (N, 1))))
    assert got[1].tolist() == [0, 0, 0, 0, 0] and got[2, 0] == got[2, 1] > 0 and got[2, 2:].tolist() == [0, 0, 0]


def test_vsd_element_offsets_past_2_to_31():
    """6 991 pairs of 480 x 640 in ONE call: the last view of depth_est / depth_gt starts past element 2^31 (8.6 GB each).  All
    zeros except a small object in the first and the last view, which are checked against the restatement; a view in between
    counts nothing."""
    from gigapose_amd import evaluate

    N, H, W, T = 6991, 480, 640, 3
    assert (N - 1) * H * W < 2 ** 31 < N * H * W
    small = random_maps(5, 2, 40, 50, T)
    de = torch.zeros(N, H, W, dtype=torch.float32, device=DEV)
    dg = torch.zeros(N, H, W, dtype=torch.float32, device=DEV)
    host_e, host_g = np.zeros((2, H, W), np.float32), np.zeros((2, H, W), np.float32)
    host_e[0, 10:50, 20:70], host_g[0, 10:50, 20:70] = small[0][0], small[1][0]
    host_e[1, 430:470, 585:635], host_g[1, 430:470, 585:635] = small[0][1], small[1][1]
    for k, n in enumerate((0, N - 1)):
        de[n], dg[n] = _t(host_e[k]), _t(host_g[k])
    dt = np.full((1, H, W), 11.0, np.float32)
    dt[0, ::7] = 0.0
    ray = eval_ref.ray_map(cases.K_CAMERA, H, W)[None]
    thr = np.tile([0.5, 1.0, 2.0], (N, 1))
    got = evaluate.vsd_counts(de, dg, _t(dt), np.zeros(N, np.int32), _t(ray), np.zeros(N, np.int32), 1.0, _t(thr))
    pick = got[[0, N - 1]].cpu().numpy()
    middle = got[1:N - 1].abs().sum().item()
    del de, dg, got
    want = eval_ref.vsd_counts(host_e, host_g, dt, [0, 0], ray, [0, 0], 1.0, thr[:2])
    np.testing.assert_array_equal(pick, want)
    assert middle == 0 and (want[:, 1] > 300).all() and not (want[0] == want[1]).all()


# ---------------------------------------------------------------------------------------------- 3. end to end on rendered meshes
H, W = 240, 320
K_SMALL = np.asarray([[300.0, 0.0, 160.0], [0.0, 302.0, 120.0], [0.0, 0.0, 1.0]])
BOX_SIZE = (60.0, 40.0, 30.0)
BOX_INFO = {"symmetries_discrete": [cases.HALF_TURN_X, cases.HALF_TURN_Y, cases.HALF_TURN_Z]}       # a box: the three half turns
DIAMETER = float(np.linalg.norm(BOX_SIZE))
ZNEAR = 1e-3


def f32_pose(R, t):
    """A pose whose entries are float32 values: what a csv of float32 poses and a float32 renderer both hold exactly."""
    return cases.rigid(R, t).astype(np.float32).astype(np.float64)


def draw(mesh, poses):
    from gigapose_amd import render

    v, f = mesh[0], mesh[1]
    return render.MeshRenderer(H, W, K_SMALL, ZNEAR)(_t(v), _t(f), None, _t(np.asarray(poses, np.float32)), colour=(255, 255, 255),
                                                     on_clipped="ignore")


def merge_depth(maps):
    """The nearest drawn surface per pixel of several depth maps (H,W) on the device."""
    big = torch.stack([torch.where(m > 0, m, torch.full_like(m, float("inf"))) for m in maps]).min(dim=0).values
    return torch.where(torch.isinf(big), torch.zeros_like(big), big)


@pytest.fixture(scope="module")
def scene():
    """A 60 x 40 x 30 box at three ground-truth poses, one per frame; frame 1 also holds an occluder box in front of a part of it.
    The frames' depth is the ground truth's render (plus the occluder's)."""
    rs = np.random.RandomState(4)
    box = meshes.box(BOX_SIZE)
    gt = np.stack([f32_pose(cases.rotation(rs), t) for t in ((-20.0, 10.0, 400.0), (15.0, -12.0, 350.0), (30.0, 25.0, 500.0))])
    depth_gt = draw(box, gt)["depth"]
    occluder = draw(meshes.box((30.0, 90.0, 10.0)), [f32_pose(np.eye(3), (25.0, -12.0, 290.0))])["depth"][0]
    frames = torch.stack([depth_gt[0], merge_depth([depth_gt[1], occluder]), depth_gt[2]]).contiguous()
    assert int(((occluder > 0) & (depth_gt[1] > 0)).sum()) > 200 and int(((occluder == 0) & (depth_gt[1] > 0)).sum()) > 200
    return dict(box=box, gt=gt, frames=frames)


def test_vsd_errors_equal_the_restatement_on_the_same_renders(scene):
    from gigapose_amd import evaluate

    rs = np.random.RandomState(6)
    gt = scene["gt"][[0, 1, 2, 1]]
    est = np.stack([g @ cases.small_motion(rs, a, s) for g, a, s in zip(gt, (0.03, 0.1, 0.3, 0.02), (2.0, 6.0, 10.0, 1.0))])
    frame = np.asarray([0, 1, 2, 1])
    out = evaluate.vsd_errors(scene["box"], est, gt, K_SMALL, scene["frames"], frame, DIAMETER, H=H, W=W, znear=ZNEAR)
    host_e, host_g = draw(scene["box"], est)["depth"].cpu().numpy(), draw(scene["box"], gt)["depth"].cpu().numpy()
    ray = eval_ref.ray_map(K_SMALL, H, W)[None]
    thr = np.asarray(evaluate.TAUS)[None, :] * np.full((4, 1), DIAMETER)
    want = eval_ref.vsd_counts(host_e, host_g, scene["frames"].cpu().numpy(), frame, ray, np.zeros(4, int), 15.0, thr)
    np.testing.assert_array_equal(out["counts"].numpy(), want)
    assert_bits(out["errors"].numpy(), eval_ref.vsd_from_counts(want), "errors")
    assert not out["clipped"].any() and out["errors"].shape == (4, 10) and out["errors"].dtype == torch.float64
    e = out["errors"].numpy()
    assert (want[:, 1] > 500).all() and (e[:, 0] >= e[:, -1]).all() and e[2, 0] > e[0, 0] and 0 < e[0, 0] < 1
    assert want[1, 0] < want[3, 0] + 2000 and want[1, 0] < int((host_g[1] > 0).sum())             # frame 1: the occluder hides a part
    # a K per pair: two groups, the second with another camera; the same as two calls
    K2 = np.stack([K_SMALL, K_SMALL * np.asarray([[1.1], [1.1], [1.0]]), K_SMALL, K_SMALL * np.asarray([[1.1], [1.1], [1.0]])])
    both = evaluate.vsd_errors(scene["box"], est, gt, K2, scene["frames"], frame, DIAMETER, H=H, W=W, znear=ZNEAR, views_per_call=1)
    np.testing.assert_array_equal(both["counts"].numpy()[[0, 2]], want[[0, 2]])
    alone = evaluate.vsd_errors(scene["box"], est[[1, 3]], gt[[1, 3]], K2[1], scene["frames"], frame[[1, 3]], DIAMETER, H=H, W=W, znear=ZNEAR)
    np.testing.assert_array_equal(both["counts"].numpy()[[1, 3]], alone["counts"].numpy())
    assert (both["counts"].numpy()[1] != want[1]).any()


def test_exact_poses_symmetric_poses_far_poses_and_poses_behind_the_camera(scene):
    from gigapose_amd import evaluate

    box, gt, frames = scene["box"], scene["gt"], scene["frames"]
    syms = evaluate.symmetry_transforms(BOX_INFO)
    assert len(syms) == 4
    frame = np.arange(3)
    # estimates equal to the ground truth: 0 / 0 exactly, VSD 0 (the occluded frame too: both renders are hidden alike)
    mssd, mspd = evaluate.pose_errors(box[0], syms, gt, gt, K_SMALL)
    assert (mssd.numpy() == 0).all() and (mspd.numpy() == 0).all()
    same = evaluate.vsd_errors(box, gt, gt, K_SMALL, frames, frame, DIAMETER, H=H, W=W, znear=ZNEAR)
    assert (same["errors"].numpy() == 0).all() and (same["counts"].numpy()[:, 0] > 500).all()
    # a pose moved by a member of the symmetry set scores the same: MSSD / MSPD to rounding (the set is closed), VSD up to the
    # pixels whose sample point lies within rounding of a silhouette edge (none are expected; 1% of the union is allowed)
    rs = np.random.RandomState(12)
    est = np.stack([g @ cases.small_motion(rs, 0.08, 4.0) for g in gt])
    base = evaluate.pose_errors(box[0], syms, est, gt, K_SMALL)
    base_vsd = evaluate.vsd_errors(box, est, gt, K_SMALL, frames, frame, DIAMETER, H=H, W=W, znear=ZNEAR)["errors"].numpy()
    assert (base[0].numpy() > 1.0).all() and (base[1].numpy() > 0.5).all() and (base_vsd[:, 0] > 0).all()
    for m in syms[1:]:
        moved = est @ m
        got = evaluate.pose_errors(box[0], syms, moved, gt, K_SMALL)
        assert np.abs(got[0].numpy() - base[0].numpy()).max() < 1e-9 * DIAMETER and np.abs(got[1].numpy() - base[1].numpy()).max() < 1e-9
        vsd = evaluate.vsd_errors(box, moved, gt, K_SMALL, frames, frame, DIAMETER, H=H, W=W, znear=ZNEAR)["errors"].numpy()
        assert np.abs(vsd - base_vsd).max() <= 0.01
    alone = evaluate.pose_errors(box[0], syms[:1], est @ syms[1], gt, K_SMALL)
    assert (alone[0].numpy() > 20.0).all()                                           # without the set the moved pose is an error
    # pushed 2 diameters away along the optical axis: every intersection pixel is bad at every tau -> exactly 1
    far = gt.copy()
    far[:, 2, 3] += np.float32(2 * DIAMETER)
    out = evaluate.vsd_errors(box, far, gt, K_SMALL, frames, frame, DIAMETER, H=H, W=W, znear=ZNEAR)
    assert (out["errors"].numpy() == 1.0).all() and (out["counts"].numpy()[:, 1] > 300).all() and not out["clipped"].any()
    # behind the camera: every triangle is dropped -> reported, error 1, no exception; a ground truth there raises
    behind = gt.copy()
    behind[1, 2, 3] = -350.0
    out = evaluate.vsd_errors(box, behind, gt, K_SMALL, frames, frame, DIAMETER, H=H, W=W, znear=ZNEAR)
    assert out["clipped"].tolist() == [False, True, False]
    assert (out["errors"].numpy()[1] == 1.0).all() and (out["errors"].numpy()[[0, 2]] == 0).all()
    with pytest.raises(ValueError, match="ground truth of pair 1"):
        evaluate.vsd_errors(box, gt, behind, K_SMALL, frames, frame, DIAMETER, H=H, W=W, znear=ZNEAR)
    d, p = evaluate.pose_errors(box[0], syms, behind, gt, K_SMALL)
    assert np.isposinf(p.numpy()[1]) and np.isfinite(d.numpy()).all() and np.isfinite(p.numpy()[[0, 2]]).all()


# ---------------------------------------------------------------------------------------------- 4. PoseScorer over a csv
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


def diameter_of(vertices):
    v = np.asarray(vertices, np.float64)
    return float(np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(axis=2).max()))


def scorer_scene():
    """Two objects (1: the box with its three half turns, 2: the asymmetric three_boxes), two images of scene 2: image 1 holds two
    boxes and one three_boxes, image 2 one of each.  The depth of an image is the render of its ground truths."""
    rs = np.random.RandomState(15)
    models = {1: dict(vertices=meshes.box(BOX_SIZE)[0], faces=meshes.box(BOX_SIZE)[1], diameter=DIAMETER, **BOX_INFO),
              2: dict(vertices=meshes.three_boxes(30.0)[0], faces=meshes.three_boxes(30.0)[1], diameter=diameter_of(meshes.three_boxes(30.0)[0]))}
    layout = {(2, 1): [(1, (-60.0, -30.0, 420.0)), (1, (50.0, 35.0, 380.0)), (2, (40.0, -45.0, 450.0))],
              (2, 2): [(2, (-30.0, 20.0, 400.0)), (1, (45.0, -10.0, 460.0))]}
    gts, cameras = {}, {}
    for key, items in layout.items():
        gts[key], maps = [], []
        for obj, t in items:
            P = f32_pose(cases.rotation(rs), t)
            gts[key].append(dict(obj_id=obj, cam_R_m2c=P[:3, :3].reshape(-1).tolist(), cam_t_m2c=P[:3, 3].tolist(), pose=P))
            maps.append(draw((models[obj]["vertices"], models[obj]["faces"]), [P])["depth"][0])
        cameras[key] = dict(cam_K=K_SMALL.reshape(-1).tolist(), depth=merge_depth(maps).cpu().numpy())
    targets = [dict(scene_id=2, im_id=1, obj_id=1, inst_count=2), dict(scene_id=2, im_id=1, obj_id=2, inst_count=1),
               dict(scene_id=2, im_id=2, obj_id=1, inst_count=1), dict(scene_id=2, im_id=2, obj_id=2, inst_count=1)]
    return models, targets, gts, cameras


def write_csv(tmp_path, name, gts, perturb, k=2):
    """One detection per ground truth, k hypotheses each, in the npz layout GigaPose.filter_and_save writes (what
    synthetic.prediction_batches imitates), merged by inout.save_predictions_from_batched_predictions.  -> the MultiHypothesis csv."""
    from gigapose_amd import inout

    out_dir = tmp_path / name
    out_dir.mkdir()
    rows = [(key, g) for key in sorted(gts) for g in gts[key]]
    for b, part in enumerate((rows[:3], rows[3:])):                                  # two batches; image 1 lies in the first
        n = len(part)
        poses = np.zeros((n, k, 4, 4), np.float32)
        scores = np.zeros((n, k), np.float32)
        for i, (key, g) in enumerate(part):
            for h in range(k):
                poses[i, h], scores[i, h] = perturb(b * 3 + i, h, g)
        np.savez(str(out_dir / f"{b}.npz"), scene_id=np.asarray([key[0] for key, _ in part], np.int32),
                 im_id=np.asarray([key[1] for key, _ in part], np.int32), object_id=np.asarray([g["obj_id"] for _, g in part], np.int32),
                 time=np.full(n, 0.05), detection_time=np.full(n, 0.1), poses=poses, scores=scores)
    paths = inout.save_predictions_from_batched_predictions(str(out_dir), "tless", "gigapose", "run", is_refined=False)
    assert paths[1].endswith("MultiHypothesis.csv")
    return paths[1]


def test_pose_scorer_over_a_csv(tmp_path):
    """Known perturbations: detection 0 exact, 1 moved by a half turn of the box (a symmetry: still exact), 2 shifted by 4 mm,
    3 shifted by 25 mm, 4 rotated by 0.5 rad; the second hypothesis of each is worse and scores lower -- except detection 3,
    whose second hypothesis is exact but scores lower, so that the order of the scores decides.  The recalls equal those computed
    from the restatement's errors (on renders pulled to the host) through the brute-force matcher."""
    from gigapose_amd import evaluate, render

    models, targets, gts, cameras = scorer_scene()
    rs = np.random.RandomState(33)
    half_turn = np.asarray(cases.HALF_TURN_Z, np.float64).reshape(4, 4)

    def perturb(i, h, g):
        P = g["pose"].copy()
        if i == 1:
            P = P @ half_turn
        elif i == 2:
            P[:3, 3] += (4.0, 0.0, 0.0)
        elif i == 3 and h == 0:
            P[:3, 3] += (0.0, 25.0, 0.0)
        elif i == 4:
            P = P @ cases.small_motion(rs, 0.5, 0.0)
        if h == 1 and i != 3:
            P = P @ cases.small_motion(rs, 0.2, 8.0)
        return P.astype(np.float32), np.float32(0.9 - 0.1 * i - 0.3 * h)

    path = write_csv(tmp_path, "perturbed", gts, perturb)
    scorer = evaluate.PoseScorer(models, targets, gts, cameras, znear=ZNEAR)
    got = scorer.score_csv(path)
    estimates = evaluate.read_estimates(path)
    assert len(estimates) == 10
    # the same errors from the restatement, pair by pair
    renderer = render.MeshRenderer(H, W, K_SMALL, ZNEAR)
    ray = eval_ref.ray_map(K_SMALL, H, W)[None]
    taus = np.asarray(evaluate.TAUS)
    tp = dict(mssd=np.zeros(10), mspd=np.zeros(10), vsd=np.zeros((10, 10)))
    total = 0
    for t, kept, g_list in scorer.pairs(estimates):
        m = models[t["obj_id"]]
        syms = evaluate.symmetry_transforms(m)
        E, G = len(kept), len(g_list)
        total += G
        assert E == t["inst_count"]
        est = np.stack([cases.rigid(e["R"], e["t"]) for e in kept for _ in g_list])
        gt = np.stack([g["pose"] for _ in kept for g in g_list])
        d2, p2 = eval_ref.mssd_mspd2(m["vertices"], syms, est, gt, np.tile(K_SMALL.reshape(9), (E * G, 1)), zmin=ZNEAR)
        depth = [renderer(_t(m["vertices"]), _t(m["faces"]), None, _t(p.astype(np.float32)), colour=(255, 255, 255))["depth"].cpu().numpy()
                 for p in (est, gt)]
        frame_depth = cameras[(t["scene_id"], t["im_id"])]["depth"][None]
        counts = eval_ref.vsd_counts(depth[0], depth[1], frame_depth, np.zeros(E * G, int), ray, np.zeros(E * G, int), 15.0,
                                     taus[None, :] * np.full((E * G, 1), m["diameter"]))
        e_vsd = eval_ref.vsd_from_counts(counts).reshape(E, G, 10)
        mssd, mspd = np.sqrt(d2).reshape(E, G), np.sqrt(p2).reshape(E, G)
        for i in range(10):
            tp["mssd"][i] += brute_force_matches(mssd.tolist(), evaluate.CORRECT_THS[i] * m["diameter"])
            tp["mspd"][i] += brute_force_matches(mspd.tolist(), 5.0 * (i + 1) * W / 640.0)
            for k in range(10):
                tp["vsd"][k, i] += brute_force_matches(e_vsd[:, :, k].tolist(), evaluate.CORRECT_THS[i])
    assert total == got["targets"] == 5 and got["clipped"] == 0
    assert got["recall_mssd"] == (tp["mssd"] / 5).tolist() and got["recall_mspd"] == (tp["mspd"] / 5).tolist()
    assert got["recall_vsd"] == (tp["vsd"] / 5).tolist()
    assert got["ar_mssd"] == float(np.mean(tp["mssd"] / 5)) and got["ar_vsd"] == float(np.mean(tp["vsd"] / 5))
    assert got["ar"] == (got["ar_mssd"] + got["ar_mspd"] + got["ar_vsd"]) / 3
    # what the perturbations must give: the two boxes of image 1 are right at every threshold (exact, and exact up to a symmetry);
    # the estimate kept for image 2's three_boxes is 25 mm off -- its exact second hypothesis scores lower and is not kept -- so
    # the tightest threshold (5% of 56 mm) misses it; recall grows with the threshold
    for name in ("recall_mssd", "recall_mspd"):
        r = got[name]
        assert 0.4 <= r[0] <= 0.8 and all(a <= b for a, b in zip(r, r[1:])) and r[-1] > r[0], (name, r)
    assert 0.4 <= got["ar_vsd"] < 1.0
    # exact poses: every recall is 1
    exact = scorer.score_csv(write_csv(tmp_path, "exact", gts, lambda i, h, g: (g["pose"].astype(np.float32), np.float32(0.9 - 0.1 * i - 0.3 * h)), k=1))
    assert exact["recall_mssd"] == [1.0] * 10 and exact["recall_mspd"] == [1.0] * 10 and exact["recall_vsd"] == [[1.0] * 10] * 10
    assert exact["ar"] == 1.0 and exact["targets"] == 5
