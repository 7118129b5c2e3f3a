"""CPU: the host half of depth refinement (gigapose_amd/refine.py, libgigapose_refine.so, include/gigapose_refine.h).

The numpy restatement of the header (gigapose_testing/refine_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_refine.py); here it is held to things that cannot share its mistakes: rational arithmetic on pixels where every
operation is exact, Rodrigues' formula for the Cayley matrix, numpy.linalg.solve for the LDL^T, and what a refiner is for --
on a small scene (three boxes in front of a wall, integer depths) it must bring three starts to below 1 % of their deviation,
rank wrong hypotheses below right ones, and stop on a sphere.  Seven subtly wrong refiners fail these checks.  Beside that: the
library against its header, the argument validation of every entry point (no GPU needed), the csv round trip."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, evaluate, refine
from gigapose_testing import refine_cases as cases
from gigapose_testing import refine_ref
from gigapose_testing.symbols import exported_symbols


# ---------------------------------------------------------------------------------------------- the library and its header
def test_refine_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_refine.so", "gpf")       # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_refine.h" and side.path == refine.REFINE_LIB_PATH
    assert sorted(protos) == ["gpf_abi_version", "gpf_accumulate", "gpf_face_normals", "gpf_last_error", "gpf_pixels_per_workgroup", "gpf_update"]
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpf_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the refine library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.gpf_last_error.restype is ctypes.c_char_p and lib.gpf_update.argtypes[5] is ctypes.c_longlong
    assert lib.gpf_update.argtypes[6:9] == [ctypes.c_double] * 3
    assert lib.gpf_abi_version() >= 1
    C = lib.gpf_pixels_per_workgroup()
    assert C == refine.pixels_per_workgroup() and C % 64 == 0 and 2 * C + 1 <= cases.H * cases.W   # the GPU tests place boxes around C and 2C
    # the constants the three statements share
    for name in ("SUMS", "RHS", "EE", "COVERED", "COUNT"):
        assert getattr(refine_ref, name) == getattr(refine, "SUMS" if name == "SUMS" else "SUM_" + name)
    for name in ("RANGE", "BAD_INDEX", "FEW", "DEGENERATE", "CLIPPED", "CONVERGED", "STOP"):
        assert getattr(refine_ref, name) == getattr(refine, name)
    header = open(_lib.INCLUDE_DIR + "/gigapose_refine.h").read()
    for name, value in (("GPF_SUMS", 32), ("GPF_SUM_RHS", 21), ("GPF_SUM_EE", 27), ("GPF_SUM_COVERED", 28), ("GPF_SUM_COUNT", 29), ("GPF_QUANTUM_BITS", 36),
                        ("GPF_RANGE", 1), ("GPF_BAD_INDEX", 2), ("GPF_FEW", 4), ("GPF_DEGENERATE", 8), ("GPF_CLIPPED", 16), ("GPF_CONVERGED", 32)):
        assert f"#define {name} {value}" in header, name


def test_refine_argument_validation_of_the_library_needs_no_gpu():
    lib = refine.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    err, ll, d = lib.gpf_last_error, ctypes.c_longlong, ctypes.c_double
    fn = lib.gpf_face_normals
    assert fn(null, 5, one, 3, one, null) == -1 and b"gpf_face_normals" in err() and b"null" in err()
    assert fn(one, 5, null, 3, one, null) == -1 and fn(one, 5, one, 3, null, null) == -1 and b"null" in err()
    for V, F in ((0, 3), (-1, 3), (5, -1)):
        assert fn(one, V, one, F, one, null) == -1 and b"bad sizes" in err(), (V, F)
    assert fn(null, 5, null, 0, null, null) == 0

    def acc(ptrs=None, F=4, M=1, N=3, H=96, W=128):
        p = [one] * 11 if ptrs is None else ptrs
        return lib.gpf_accumulate(p[0], p[1], F, p[2], p[3], p[4], M, p[5], p[6], p[7], p[8], N, H, W, p[9], p[10], null)

    for i in range(11):                                          # each pointer in turn
        p = [one] * 11
        p[i] = null
        assert acc(p) == -1 and b"gpf_accumulate" in err() and b"null" in err(), i
    for kw in (dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=2048, W=2049), dict(F=-1), dict(M=0)):
        assert acc(**kw) == -1 and b"bad sizes" in err(), kw
    p = [one] * 11
    p[9] = ctypes.c_void_p(12)
    assert acc(p) == -1 and b"aligned" in err()
    assert acc([null] * 11, N=0) == 0 and acc([null] * 11, N=0, H=0) == -1   # N = 0: nothing to do, but the sizes are still checked

    def upd(ptrs=None, N=3, min_points=ll(10), min_pivot=d(1e-3), damping=d(0.0), tol2=d(1e-12)):
        p = [one] * 7 if ptrs is None else ptrs
        return lib.gpf_update(p[0], p[1], p[2], p[3], N, min_points, min_pivot, damping, tol2, p[4], p[5], p[6], null)

    for i in (0, 2, 4, 5, 6):
        p = [one] * 7
        p[i] = null
        assert upd(p) == -1 and b"gpf_update" in err() and b"null" in err(), i
    for kw in (dict(N=-1), dict(N=65536)):
        assert upd(**kw) == -1 and b"bad sizes" in err(), kw
    for kw in (dict(min_points=ll(-1)), dict(min_pivot=d(-1.0)), dict(min_pivot=d(math.inf)), dict(damping=d(math.nan)), dict(tol2=d(math.nan)),
               dict(tol2=d(-1.0))):
        assert upd(**kw) == -1 and b"must be" in err(), kw
    assert upd([null] * 7, N=0) == 0


def test_refine_argument_validation_of_the_python_layer_needs_no_gpu(tmp_path):
    v, f = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="vertices"):
        refine.face_normals(v.double(), f)
    with pytest.raises(ValueError, match="faces"):
        refine.face_normals(v, f.long())
    with pytest.raises(ValueError, match="V = 0"):
        refine.face_normals(v[:0], f)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        refine.face_normals(v, f)
    N, H, W = 2, 8, 8
    a = dict(vis=torch.zeros(N, H, W, dtype=torch.int64), c=torch.zeros(4, 3, dtype=torch.float64), poses=torch.eye(4, dtype=torch.float64).repeat(N, 1, 1),
             K=torch.zeros(N, 9, dtype=torch.float64), depth=torch.zeros(1, H, W), frame=torch.zeros(N, dtype=torch.int32),
             box=torch.zeros(N, 4, dtype=torch.int32), gate=torch.ones(N, dtype=torch.float64), scale=torch.ones(N, dtype=torch.float64))
    for what, bad in (("vis", a["vis"].int()), ("c", a["c"].float()), ("poses", a["poses"][:1]), ("K", a["K"][:, :8]), ("depth", a["depth"][:, :4]),
                      ("frame", a["frame"].long()), ("box", a["box"][:, :3]), ("gate", a["gate"].float()), ("scale", a["scale"][:1])):
        with pytest.raises(ValueError, match=what):
            refine.accumulate(**dict(a, **{what: bad}))
    with pytest.raises(ValueError, match="must be a torch tensor"):
        refine.accumulate(**dict(a, box=a["box"].numpy()))
    with pytest.raises(ValueError, match="2\\^22"):
        refine.accumulate(**dict(a, vis=torch.empty(N, 2048, 2049, dtype=torch.int64), depth=torch.empty(1, 2048, 2049)))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        refine.accumulate(**a)
    u = dict(sums=torch.zeros(N, 32, dtype=torch.int64), clipped=None, scale=a["scale"], start=None, poses=a["poses"].clone(),
             poses32=a["poses"].float(), state=torch.zeros(N, dtype=torch.int32))
    for what, bad in (("sums", u["sums"][:, :30]), ("clipped", torch.zeros(N)), ("start", a["poses"].float()), ("poses32", a["poses"]),
                      ("state", torch.zeros(N))):
        with pytest.raises(ValueError, match=what):
            refine.update(**dict(u, **{what: bad}))
    for kw in (dict(min_points=-1), dict(min_points=2.5), dict(min_pivot=-1.0), dict(damping=math.inf), dict(tol2=math.nan)):
        with pytest.raises(ValueError, match="must be"):
            refine.update(**u, **kw)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        refine.update(**u)
    models = {1: dict(vertices=np.zeros((5, 3), np.float32), faces=np.zeros((4, 3), np.int32), diameter=10.0)}
    cameras = {(1, 1): dict(cam_K=cases.K, depth=np.zeros((8, 8), np.float32))}
    for kw, match in ((dict(iters=-1), "iters"), (dict(gate=-1.0), "gate"), (dict(box="tight"), "box"), (dict(min_pivot=-1.0), "min_pivot")):
        with pytest.raises(ValueError, match=match):
            refine.DepthRefiner(models, cameras, **kw)
    with pytest.raises(ValueError, match="no cameras"):
        refine.DepthRefiner(models, {})
    with pytest.raises(ValueError, match="diameter"):
        refine.DepthRefiner({1: dict(models[1], diameter=None)}, cameras)
    with pytest.raises(ValueError, match="differ in size"):
        refine.DepthRefiner(models, {**cameras, (1, 2): dict(cam_K=cases.K, depth=np.zeros((8, 9), np.float32))})
    r = refine.DepthRefiner(models, cameras, device="cpu")
    est = dict(scene_id=1, im_id=1, obj_id=1, score=0.5, R=np.eye(3), t=np.asarray([0.0, 0.0, 100.0]))
    with pytest.raises(ValueError, match="no camera"):
        r.refine([dict(est, im_id=2)])
    with pytest.raises(ValueError, match="no model"):
        r.refine([dict(est, obj_id=2)])
    with pytest.raises(ValueError, match="boxes"):
        r.refine([est], boxes=[(0, 0, 1)])
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        r.refine([est])
    assert r.pairs_per_call == min(65535, (1 << 30) // (8 * 8 * 8)) and refine.DepthRefiner(models, cameras, pairs_per_call=2).pairs_per_call == 2


# ---------------------------------------------------------------------------------------------- exact arithmetic
def restated_exact_sums(variant=None):
    keys, dm, px, py = cases.exact_pixels()
    terms, status, info = refine_ref.pixel_terms(keys, dm, px, py, cases.EXACT_NORMALS, cases.EXACT_POSE, cases.EXACT_K, cases.EXACT_GATE,
                                                 cases.EXACT_SCALE, variant)
    return terms, status, info


def test_restatement_equals_rational_arithmetic_on_exact_pixels():
    keys, dm, px, py = cases.exact_pixels()
    want = cases.rational_sums(keys, dm, px, py)
    terms, status, info = restated_exact_sums()
    assert terms.sum(axis=0).tolist() == want and status == 0
    # the case says what it claims: the pixel ON the gate is kept, the next f32 above is not; most pixels count; the quantisation rounds
    assert info["assoc"][:4].tolist() == [True, False, False, False] and want[28] == 39 and 15 <= want[29] < 37
    exact = info["terms"][info["assoc"]] * 2.0 ** 36
    assert (exact != np.rint(exact)).any(), "no term has a bit below the quantum: floor and rint could not be told apart"
    for o in range(28):
        assert terms[:, o].any(), o


# ---------------------------------------------------------------------------------------------- the step
def rodrigues(omega):
    n = float(np.linalg.norm(omega))
    return cases.rot(omega, np.rad2deg(2.0 * math.atan(n / 2.0))) if n else np.eye(3)


def test_cayley_is_a_rotation_and_equals_rodrigues():
    rs = np.random.RandomState(3)
    for scale in (1e-9, 1e-3, 0.1, 1.0, 3.0):
        for _ in range(5):
            omega = rs.standard_normal(3) * scale
            Q = refine_ref.cayley(omega)
            assert np.abs(Q @ Q.T - np.eye(3)).max() < 8 * np.finfo(np.float64).eps
            assert abs(np.linalg.det(Q) - 1.0) < 8 * np.finfo(np.float64).eps
            assert np.abs(Q - rodrigues(omega)).max() < 16 * np.finfo(np.float64).eps
    assert (refine_ref.cayley([0.0, 0.0, 0.0]) == np.eye(3)).all()
    assert np.abs(refine_ref.cayley([0.0, 0.0, 2.0]) - cases.rot([0, 0, 1], 90)).max() < 1e-15      # |omega| = 2: a quarter turn


def test_ldl_solves_the_accumulated_systems_and_flags_every_pivot():
    out = cases.run("boxes", "right", iters=0)                   # the sums at the three starts
    for row in out["sums"]:
        A, rhs = refine_ref.normal_equations(row)
        x, pivots, bad = refine_ref.ldl_solve(A, rhs, 1e-3 * float(row[refine_ref.COUNT]))
        assert bad is None and min(pivots) > 1e-3 * float(row[refine_ref.COUNT])
        want = np.linalg.solve(A, rhs)
        assert np.abs(np.asarray(x) - want).max() <= 1e-9 * np.abs(want).max()
    for j in range(6):
        A, L, D = cases.integer_ldl(j, j + 1)
        x, pivots, bad = refine_ref.ldl_solve(A, np.ones(6), 0.0)
        assert bad == j and x is None and pivots == D[:j + 1].tolist()
        A[j, j] -= 1.0                                           # ... and a negative one
        assert refine_ref.ldl_solve(A, np.ones(6), 0.0)[2] == j
    A, L, D = cases.integer_ldl()
    x, pivots, bad = refine_ref.ldl_solve(A, A @ np.arange(1.0, 7.0), 0.0)
    assert bad is None and pivots == D.tolist() and x == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]              # exact on integers


def test_update_on_planted_sums():
    sums, want, state, clipped = cases.planted_sums()
    n = len(sums)
    rs = np.random.RandomState(9)
    start = np.stack([cases.rigid(cases.rot(rs.standard_normal(3), 30 * i), rs.uniform(-50, 50, 3)) for i in range(n)])
    poses = np.stack([cases.rigid(cases.rot(rs.standard_normal(3), 20 + i), rs.uniform(-50, 50, 3)) for i in range(n)])
    new, new32, got = refine_ref.update(sums, clipped, np.full(n, 100.0), start, 32, 1e-3, 0.0, 1e-4, poses, state)
    assert got.tolist() == want.tolist()
    assert (new[9] == poses[9]).all()                            # stopped before: untouched
    for i in (2, 3, 4, 5, 6, 7, 8, 10):
        assert (new[i] == start[i]).all(), i                     # stops now: the input pose comes back
    kept, _, _ = refine_ref.update(sums, clipped, np.full(n, 100.0), None, 32, 1e-3, 0.0, 1e-4, poses, state)
    assert (kept[2:] == poses[2:]).all() and (kept[:2] == new[:2]).all()
    for i in (0, 1):
        A, rhs = refine_ref.normal_equations(sums[i])
        xi = np.linalg.solve(A, rhs)
        R = rodrigues(xi[:3]) @ poses[i][:3, :3]
        assert np.abs(new[i][:3, :3] - R).max() < 1e-12 and np.abs(new[i][:3, 3] - (poses[i][:3, 3] + 100.0 * xi[3:])).max() < 1e-9
        assert (new[i][3] == [0, 0, 0, 1]).all()
    assert (new32 == new.astype(np.float32)).all()
    assert refine_ref.update(sums, clipped, np.full(n, 100.0), start, 32, 1e-3, 0.0, 0.0, poses, state)[2][0] == 0     # tol2 = 0: never converged


# ---------------------------------------------------------------------------------------------- invariances of the integer sums
def test_sums_do_not_depend_on_order_box_or_chunks():
    v, f = cases.mesh("boxes")
    c = refine_ref.face_normals(v, f)
    pose = cases.starts()[1]
    vis = cases.draw(v, f, pose)
    depth = cases.sensor_depth("boxes")
    args = (c, pose, cases.K, cases.GATE, cases.SCALE)
    py, px = np.meshgrid(np.arange(cases.H), np.arange(cases.W), indexing="ij")
    terms, status, info = refine_ref.pixel_terms(vis, depth, px, py, *args)
    whole = terms.sum(axis=0)
    assert status == 0 and whole[refine_ref.COUNT] > 200
    rs = np.random.RandomState(1)
    order = rs.permutation(vis.size)
    shuffled, _, _ = refine_ref.pixel_terms(vis.reshape(-1)[order], depth.reshape(-1)[order], px.reshape(-1)[order], py.reshape(-1)[order], *args)
    assert (shuffled.sum(axis=0) == whole).all() and (shuffled == terms[order]).all()
    for parts in (2, 3, 7, 64):
        cuts = np.sort(rs.randint(0, vis.size, parts - 1))
        assert (sum(part.sum(axis=0) for part in np.split(shuffled, cuts)) == whole).all()
    ys, xs = np.nonzero(vis != refine_ref.raster_ref.EMPTY_KEY)
    tight = np.asarray([[xs.min(), ys.min(), xs.max(), ys.max()]])
    one = lambda box: refine_ref.accumulate(vis[None], c, pose[None], cases.K[None], depth[None], [0], box, [cases.GATE], [cases.SCALE])[0][0]
    assert (one(tight)[:30] == whole).all() and (one(cases.whole_frame(1))[:30] == whole).all()
    assert (one(tight + [[-5, -200, 300, 7]])[:30] == whole).all() and not one([[5, 5, 4, 90]]).any() and not one([[200, 0, 300, 50]]).any()
    # a float sum of the same terms does depend on the order: that is what the quantisation is for
    t = info["terms"][info["assoc"]][:, 0]
    assert len({float(np.sum(t[rs.permutation(len(t))])) for _ in range(20)}) > 1


# ---------------------------------------------------------------------------------------------- what a refiner is for
def convergence(variant=None):
    """-> the end deviation over the start deviation of the three starts (inf for a pair that stopped)."""
    v, _ = cases.mesh("boxes")
    out = cases.run("boxes", "right", variant)
    return [cases.deviation(v, p) / cases.deviation(v, s) if not st & refine_ref.STOP else math.inf
            for p, s, st in zip(out["poses"], cases.starts(), out["state"])], out


def test_three_starts_converge_to_below_one_percent():
    v, _ = cases.mesh("boxes")
    begin = [cases.deviation(v, s) for s in cases.starts()]
    assert [round(b, 1) for b in begin] == [8.6, 16.4, 38.6]
    ratios, out = convergence()
    print("start", begin, "end", [cases.deviation(v, p) for p in out["poses"]], "ratios", ratios)
    assert max(ratios) < 0.01
    s = out["sums"]
    assert (s[:, refine_ref.COVERED] == s[:, refine_ref.COUNT]).all() and (s[:, refine_ref.COUNT] > 300).all()   # every covered pixel is associated
    assert not out["status"].any() and int(np.abs(s).max()) < 2 ** 44
    # unrounded depth: the end is the fixed point itself
    n = 3
    fine = refine_ref.refine(v, cases.mesh("boxes")[1], cases.starts(), np.tile(cases.K, (n, 1)), cases.sensor_depth("boxes", 0, False)[None],
                             np.zeros(n, np.int32), cases.whole_frame(n), np.full(n, cases.GATE), np.full(n, cases.SCALE), cases.ITERS, 32, 1e-3, 0.0,
                             1e-12, cases.H, cases.W)
    assert max(cases.deviation(v, p) for p in fine["poses"]) < 0.005


def test_wrong_hypotheses_rank_below_right_ones():
    right, wrong = cases.quality(cases.run("boxes", "right")), cases.quality(cases.run("boxes", "wrong"))
    print("right: inliers / covered", right[0], "rms", right[1], "| wrong:", wrong[0], wrong[1])
    assert wrong[0].max() < right[0].min() and wrong[1].min() > right[1].max()
    assert right[0].min() == 1.0 and right[1].max() < 0.35       # integer depths: 1/sqrt(12) = 0.29 along the ray at most


def test_a_sphere_stops_as_degenerate_and_converges_with_a_lower_bar():
    """A sphere does not constrain the rotation: at min_pivot = 1e-3 every start stops as degenerate with its pose unchanged; at
    1e-5 the CENTRE converges to within 0.02.  That bar is held on the depth as rendered: integer depths move the fixed point
    itself by 0.027 on this scene (a run started AT the ground truth ends there), which is the data's doing, so on them the bar is
    that the three starts end within 0.02 of that fixed point."""
    stopped = cases.run("sphere", "right")
    assert (stopped["state"] & refine_ref.STOP == refine_ref.DEGENERATE).all() and (stopped["poses"] == cases.starts()).all()
    loose = cases.run("sphere", "right", min_pivot=1e-5, rounded=False)
    centre = [float(np.linalg.norm(p[:3, 3] - cases.GT[:3, 3])) for p in loose["poses"]]
    integer = cases.run("sphere", "right", min_pivot=1e-5)
    v, f = cases.mesh("sphere")
    fixed = refine_ref.refine(v, f, cases.GT[None], cases.K[None], cases.sensor_depth("sphere")[None], [0], cases.whole_frame(1), [cases.GATE], [cases.SCALE],
                              cases.ITERS, 32, 1e-5, 0.0, 1e-12, cases.H, cases.W)["poses"][0]
    off = [float(np.linalg.norm(p[:3, 3] - fixed[:3, 3])) for p in integer["poses"]]
    print("centre error", centre, "| integer depths: from the fixed point", off, "the fixed point from the truth", np.linalg.norm(fixed[:3, 3] - cases.GT[:3, 3]))
    assert not (loose["state"] & refine_ref.STOP).any() and max(centre) < 0.02
    assert not (integer["state"] & refine_ref.STOP).any() and max(off) < 0.02
    first = cases.run("sphere", "right", iters=0)["sums"]
    for row in first:
        _, pivots, _ = refine_ref.ldl_solve(*refine_ref.normal_equations(row), 0.0)
        assert max(pivots[:3]) < 1e-3 * float(row[refine_ref.COUNT]) < min(pivots[3:])


@pytest.mark.parametrize("variant", refine_ref.VARIANTS)
def test_the_checks_reject_wrong_refiners(variant):
    """y x m written as m x y; a = omega (twice the angle); t += tau without the scale; y taken about the camera's origin while the
    rotation is applied about the object's; the weight 1/|m|; floor for rint; < for <= at the gate."""
    keys, dm, px, py = cases.exact_pixels()
    exact_ok = restated_exact_sums(variant)[0].sum(axis=0).tolist() == cases.rational_sums(keys, dm, px, py)
    converges = max(convergence(variant)[0]) < 0.01
    must_fail = {"cross_swapped": "both", "full_omega": "convergence", "unscaled_t": "convergence", "camera_origin": "both",
                 "weight_inv_norm": "both", "floor": "exact", "strict_gate": "exact"}[variant]
    if must_fail in ("exact", "both"):
        assert not exact_ok
    if must_fail in ("convergence", "both"):
        assert not converges


# ---------------------------------------------------------------------------------------------- csv
def test_write_estimates_round_trip(tmp_path):
    rs = np.random.RandomState(2)
    est = [dict(scene_id=int(rs.randint(1, 50)), im_id=int(rs.randint(0, 1000)), obj_id=int(rs.randint(1, 30)), score=float(rs.uniform()),
                R=cases.rot(rs.standard_normal(3), rs.uniform(0, 180)), t=rs.uniform(-1000, 1000, 3)) for _ in range(20)]
    est[3]["time"] = 0.125
    est[4].update(status=8, inliers=5, covered=9, rms=float("nan"))            # what refine() adds is not written
    path = refine.write_estimates(tmp_path / "refined.csv", est)
    back = evaluate.read_estimates(path)
    assert len(back) == 20
    for a, b in zip(est, back):
        assert set(b) == {"scene_id", "im_id", "obj_id", "score", "R", "t"}
        assert all(a[k] == b[k] for k in ("scene_id", "im_id", "obj_id", "score"))
        assert (a["R"].view(np.uint64) == b["R"].view(np.uint64)).all() and (a["t"].view(np.uint64) == b["t"].view(np.uint64)).all()
    lines = open(path).read().split("\n")
    assert lines[0] == "scene_id,im_id,obj_id,score,R,t,time" and lines[4].endswith(",0.125") and lines[1].endswith(",-1")
    refine.write_estimates(path, back)
    again = evaluate.read_estimates(path)
    assert all((a["R"] == b["R"]).all() and (a["t"] == b["t"]).all() and a["score"] == b["score"] for a, b in zip(back, again))
    with pytest.raises(ValueError, match="9 / 3"):
        refine.write_estimates(path, [dict(est[0], R=np.eye(2))])
