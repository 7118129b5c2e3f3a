"""GPU: untextured mesh + poses + point lights -> lit RGBA renders and depth (libgigapose_shade.so, gigapose_amd/shade.py).

The two kernels against the numpy restatement (gigapose_testing/shade_ref.py, written from the header) bit for bit: vertex normals
around thread and workgroup edges, the 70-fan, every flag, permuted faces, a second call into the same buffers; the shader on
three meshes, two frames, both modes, 0 / 1 / 8 / 16 lights and three table sizes, with planted keys, zero and NaN normals, lights
in the surface's plane and at a surface point, NaN and infinite lights and poses.  Then ShadedMeshRenderer (the restatement's
render, chunking, no light = MeshRenderer), a render buffer past 2^32 bytes, and ShadedMeshTemplates -> set_template_data ->
predict against RenderedTemplates on the saved PNGs.  The last proves plumbing, not accuracy: the model is randomly initialised."""
import numpy as np
import pytest
import torch

from gigapose_testing import factory, meshes, raster_ref
from gigapose_testing import shade_ref as sr
from gigapose_testing import synthetic as syn
from gigapose_testing.gpu_cases import DEV, K_SMALL, ZNEAR, assert_bits, grey, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. gpl_vertex_normals
def normals_on_device(v, f, unit, out=None):
    from gigapose_amd import shade

    acc, flags, n = shade.vertex_normals_raw(_t(v), _t(f), unit, out=out)
    return acc.cpu().numpy(), flags.cpu().numpy(), n.cpu().numpy()


def assert_normals(got, want, what):
    for g, w, name in zip(got, want, ("acc", "flags", "normals")):
        assert_bits(g, w, f"{what}: {name}")


def test_vertex_normals_equal_the_restatement_around_thread_and_workgroup_edges():
    """Random vertices and random faces (repeated corners, degenerate faces and a few indices out of range included), V from 1 to
    2 049 and F from 0 to 4 096: one thread short of a wave, of a workgroup, one beyond, several workgroups."""
    rs = np.random.RandomState(17)
    for V, F in ((1, 0), (1, 3), (2, 1), (63, 64), (64, 63), (65, 65), (255, 256), (256, 255), (257, 257), (1000, 0), (2048, 4095), (2049, 4096)):
        v = rs.uniform(-40, 40, (V, 3)).astype(np.float32)
        f = rs.randint(0, V, (F, 3)).astype(np.int32)
        if F > 8:
            f[rs.randint(F, size=3), rs.randint(3, size=3)] = (V, -1, 2 ** 31 - 1)
        unit = 2.0 ** 20
        want = sr.vertex_normals(v, f, unit)
        assert_normals(normals_on_device(v, f, unit), want, f"V = {V}, F = {F}")
        assert not (want[1] & sr.RANGE).any() and (V < 60 or F == 0 or (want[1] == 0).sum() > V // 4)


def test_the_fan_every_flag_permuted_faces_and_a_second_call():
    from gigapose_amd import shade

    v, f = sr.fan(70)
    want = sr.vertex_normals(v, f, 2.0)
    assert_normals(normals_on_device(v, f, 2.0), want, "the fan of 70")
    assert int(want[0][0, 2]) > 70 * 1500
    for name, (gv, gf, unit, flags) in sr.guard_cases().items():
        got = normals_on_device(gv, gf, unit)
        assert_normals(got, sr.vertex_normals(gv, gf, unit), name)
        assert got[1].tolist() == flags, name
    rs = np.random.RandomState(23)
    v, f, _ = meshes.icosphere(2, 0.7)
    unit = shade.normal_unit(v)
    base = normals_on_device(v, f, unit)
    g = np.stack([np.roll(row, rs.randint(3)) for row in f[rs.permutation(len(f))]]).astype(np.int32)
    assert_normals(normals_on_device(v, g, unit), base, "faces permuted, corners rotated")
    assert_normals(base, sr.vertex_normals(v, f, unit), "icosphere")
    # the call initialises its buffers: garbage first, then two calls into the same three tensors
    out = (torch.full((len(v), 3), 0x5A5A5A5A5A, dtype=torch.int64, device=DEV), torch.full((len(v),), 7, dtype=torch.int32, device=DEV),
           torch.full((len(v), 3), float("nan"), dtype=torch.float64, device=DEV))
    assert_normals(normals_on_device(v, f, unit, out=out), base, "over garbage")
    assert_normals(normals_on_device(v, f, unit, out=out), base, "second call into the same buffers")
    assert_bits(shade.vertex_normals(_t(v), _t(f)), base[2], "vertex_normals")
    bad = v.copy()
    bad[5, 1] = np.inf
    with pytest.raises(ValueError, match=r"vertex \d+ = .* belongs to a face whose cross product is not finite"):
        shade.vertex_normals(_t(bad), _t(f))


# ---------------------------------------------------------------------------------------------- 2. gpl_shade
def scenes():
    """name -> (vertices, faces, colours, poses (3,4,4)): a box of six colours, three_boxes painted grey, an icosphere of level 2
    with its direction colours."""
    rs = np.random.RandomState(41)

    def views(depths, off):
        return np.stack([pose(rotation(rs), (off[0], off[1], d)) for d in depths]).astype(np.float32)

    b, t, i = meshes.box((1.0, 0.6, 0.3)), meshes.three_boxes(), meshes.icosphere(2, 0.8)
    return {"box": b + (views((1.6, 3.0, 9.0), (0.05, -0.03)),), "three_boxes": (t[0], t[1], grey(t[0])) + (views((3.2, 5.0, 12.0), (-0.1, 0.05)),),
            "icosphere": i + (views((1.8, 4.0, 20.0), (0.02, 0.04)),)}


def some_lights(L, rs):
    """L lights about the camera, the first behind it, in model units of a scene a few units deep."""
    rows = np.concatenate([rs.uniform(-2, 2, (L, 2)), rs.uniform(-1.5, 1.0, (L, 1)), rs.uniform(0.5, 6.0, (L, 1))], axis=1)
    return rows.astype(np.float64)


def shade_both(vis, xy, z, f, c, v, n, P, K, lights, ambient, tables, mode):
    """The kernel and the restatement on the same keys -> ((rgba, depth, unlit) got, want)."""
    from gigapose_amd import shade

    got = shade.shade(vis, _t(xy), _t(z), _t(f), _t(c), _t(v), _t(n), _t(P), K, lights, ambient, _t(tables[0]), _t(tables[1]), mode)
    torch.cuda.synchronize()
    keys = vis.cpu().numpy().view(np.uint64)
    want = sr.shade(keys, xy, z, f, c, v, n, P, K, lights, ambient, tables[0], tables[1], mode)
    return tuple(g.cpu().numpy() for g in got), want


def assert_shaded(got, want, what):
    for g, w, name in zip(got, want, ("rgba", "depth", "unlit")):
        assert_bits(g, w, f"{what}: {name}")


@pytest.fixture(scope="module")
def tables():
    from gigapose_amd import shade

    return {256: shade.linear_tables(256), 4096: shade.srgb_tables(4096), 65536: shade.srgb_tables(65536)}


@pytest.mark.parametrize("frame", [(48, 64), (17, 33)], ids=["64x48", "33x17"])
def test_shade_equals_the_restatement(frame, tables):
    """Box, three_boxes and icosphere at 3 views each, both modes; the number of lights and the table size rotate through 0, 1, 8,
    16 and 256, 4096, 65 536 so that every value meets both modes and every mesh.  Keys from the kernel's own raster
    (tests/test_gpu_render.py holds those to raster_ref)."""
    from gigapose_amd import render, shade

    H, W = frame
    K = np.asarray([[0.9 * W, 0.25, (W - 1) / 2 + 0.3], [0, 0.95 * W, (H - 1) / 2 - 0.2], [0, 0, 1]], np.float32)
    rs = np.random.RandomState(H)
    seen, turn = set(), 0
    for shift, (name, (v, f, c, P)) in enumerate(scenes().items()):
        xy, z = raster_ref.project(v, P, K, ZNEAR)
        vis, clipped = render.raster(_t(xy), _t(z), _t(f), H, W)
        assert clipped.tolist() == [0, 0, 0]
        n = sr.vertex_normals(v, f, shade.normal_unit(v))[2]
        for mode in (sr.SMOOTH, sr.FLAT):
            for k in range(2):
                L, T = (0, 1, 8, 16)[(turn + 2 * shift) % 4], (256, 4096, 65536)[turn % 3]
                turn += 1
                seen.add((mode, L))
                got, want = shade_both(vis, xy, z, f, c, v, n, P, K, some_lights(L, rs), 0.05 if L else 0.8, tables[T], mode)
                assert_shaded(got, want, f"{name}, mode {mode}, {L} lights, T = {T}")
                a = got[0][..., 3]
                assert set(np.unique(a)) == {0, 255} and (got[1][a == 0] == 0).all() and (got[0][a == 0] == 0).all() and (got[1][a == 255] > 0).all()
                assert got[2].tolist() == [0, 0, 0] and (a == 255).sum() > (150 if H > 20 else 20)
                if L:
                    assert len(np.unique(got[0][a == 255][:, :3].astype(np.int64) @ (1, 256, 65536))) > (3 if name == "three_boxes" else 6)
    assert seen == {(m, L) for m in (0, 1) for L in (0, 1, 8, 16)}


def test_planted_keys_and_unusable_normals(tables):
    """One view of the icosphere in a 64 x 48 frame, its key buffer edited by hand: an uncovered key inside the drawing; a face
    index >= F; a face that names a vertex >= V and one that names -1; covered keys at the first and the last lane of the
    first wave (pixels 0 and 63), at pixel 64 and in the last pixel of the frame, all outside the triangle they name (the edge
    values are negative there: the arithmetic is defined all the same).  Then the normals of some vertices are zero, NaN and
    infinite: every pixel of a face that loses its normal is counted in unlit and shows the ambient term alone."""
    from gigapose_amd import render

    H, W = 48, 64
    v, f, c = meshes.icosphere(2, 0.8)
    P = pose(rotation(np.random.RandomState(77)), (0.0, 0.0, 2.2))[None].astype(np.float32)
    K = np.asarray([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], np.float32)
    f = np.concatenate([f, [(0, 1, len(v)), (-1, 2, 3)]]).astype(np.int32)           # two faces nobody can draw
    F = len(f)
    xy, z = raster_ref.project(v, P, K, ZNEAR)
    vis, clipped = render.raster(_t(xy), _t(z), _t(f), H, W)
    assert clipped.tolist() == [2]
    keys = vis.cpu().numpy().view(np.uint64).copy()
    owner = np.where(keys[0] != raster_ref.EMPTY_KEY, (keys[0] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    assert owner[24, 32] >= 0 and owner[0, 0] == -1 and owner[H - 1, W - 1] == -1 and (owner >= 0).sum() > 800
    depth_bits = np.uint64(np.float32(2.5).view(np.uint32)) << np.uint64(32)
    keys[0, 24, 32] = raster_ref.EMPTY_KEY
    keys[0, 24, 33] = depth_bits | np.uint64(F)
    keys[0, 24, 34] = depth_bits | np.uint64(0xFFFFFFFE)
    keys[0, 25, 32] = depth_bits | np.uint64(F - 2)
    keys[0, 25, 33] = depth_bits | np.uint64(F - 1)
    for (y, x), face in (((0, 0), 3), ((0, 63), 17), ((1, 0), 40), ((H - 1, W - 1), int(owner[24, 30]))):
        keys[0, y, x] = depth_bits | np.uint64(face)
    planted = _t(keys.view(np.int64))
    n = sr.vertex_normals(v, f, 2.0 ** 30)[2]
    lights = some_lights(8, np.random.RandomState(1))
    for mode in (sr.SMOOTH, sr.FLAT):
        got, want = shade_both(planted, xy, z, f, c, v, n, P, K, lights, 0.1, tables[4096], mode)
        assert_shaded(got, want, f"planted keys, mode {mode}")
        rgba = got[0][0]
        for y, x in ((24, 32), (24, 33), (24, 34), (25, 32), (25, 33)):
            assert rgba[y, x].tolist() == [0, 0, 0, 0] and got[1][0, y, x] == 0
        for y, x in ((0, 0), (0, 63), (1, 0), (H - 1, W - 1)):
            assert rgba[y, x, 3] == 255 and got[1][0, y, x] == np.float32(2.5)
    broken = n.copy()
    faces_seen, counts = np.unique(owner[owner >= 0], return_counts=True)
    big = faces_seen[np.argsort(-counts)][:4]
    broken[f[big[0]]] = 0.0                                          # all three corners: mm = 0
    broken[f[big[1]][0]] = np.nan
    broken[f[big[2]][1]] = np.inf
    broken[f[big[3]][2]] = -0.0
    got, want = shade_both(vis, xy, z, f, c, v, broken, P, K, lights, 0.1, tables[4096], sr.SMOOTH)
    assert_shaded(got, want, "zero, NaN and infinite normals")
    touched = np.isin(f[:, :3], np.concatenate([f[big[1]][:1], f[big[2]][1:2]])).any(axis=1)
    dark = np.isin(owner, np.nonzero(touched)[0]) | (owner == big[0])
    assert got[2].tolist() == [int(dark.sum())] and dark.sum() > 60
    ambient_only, _ = shade_both(vis, xy, z, f, c, v, n, P, K, [], 0.1, tables[4096], sr.SMOOTH)
    assert (got[0][0][dark] == ambient_only[0][0][dark]).all() and (got[0][0][(owner >= 0) & ~dark] != ambient_only[0][0][(owner >= 0) & ~dark]).any()


def test_lights_in_the_plane_at_a_surface_point_and_not_finite(tables):
    """A plane facing the camera at z = 4 (the scene of tests/test_shade_host.py): lights behind it, exactly in its plane (md == 0)
    and exactly at the surface point of the centre pixel (dd == 0) add nothing -- every pixel shows the ambient term.  Then NaN
    and infinite light positions and intensities, and NaN / infinite pose entries: the kernel's bytes are the restatement's."""
    from gigapose_amd import render

    H, W = 17, 33
    v = np.asarray([(-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0)], np.float32)
    f = np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)
    c = np.asarray([(200, 100, 50), (60, 120, 240), (255, 255, 255), (10, 20, 30)], np.uint8)
    K = np.asarray([[16.0, 0, 16.0], [0, 16.0, 8.0], [0, 0, 1]], np.float32)
    P = pose(np.eye(3), (0, 0, 4.0))[None].astype(np.float32)
    xy, z = raster_ref.project(v, P, K, ZNEAR)
    vis, _ = render.raster(_t(xy), _t(z), _t(f), H, W)
    n = sr.vertex_normals(v, f, 1.0)[2]
    nothing = [(0.5, 0.2, 6.0, 1e6), (0.0, 0.0, 4.0, 1e6), (1.0, 1.0, 4.0, 1e6)]
    for mode in (sr.SMOOTH, sr.FLAT):
        got, want = shade_both(vis, xy, z, f, c, v, n, P, K, nothing, 0.25, tables[256], mode)
        assert_shaded(got, want, f"lights that add nothing, mode {mode}")
        ambient, _ = shade_both(vis, xy, z, f, c, v, n, P, K, [], 0.25, tables[256], mode)
        assert_bits(got[0], ambient[0], "rgba under lights that add nothing")
        assert (got[0][..., 3] == 255).sum() > 200
        lit, _ = shade_both(vis, xy, z, f, c, v, n, P, K, [(0.0, 0.0, 0.0, 8.0)], 0.0, tables[256], mode)
        assert lit[0][0, 8, 16].tolist() == [sr_byte(c, 0.5, k) for k in range(3)] + [255]      # E = 1/2 exactly at the centre pixel
        weird = [(np.nan, 0, 0, 1.0), (0, 0, 0, np.inf), (np.inf, 0, 0, 1.0), (0, 0, 0, np.nan), (0, 0, 1, -np.inf), (0.3, 0.1, 1.0, 2.0), (1e200, 0, 0, 1e300),
                 (1e-200, 0, 4.0, 1e-300)]
        for l in range(len(weird)):
            got, want = shade_both(vis, xy, z, f, c, v, n, P, K, weird[l:l + 2], 0.1, tables[65536], mode)
            assert_shaded(got, want, f"lights {l}, {l + 1} of the odd ones, mode {mode}")
        for entry, value in (((0, 0), np.nan), ((1, 2), np.inf), ((2, 2), -np.inf), ((0, 3), np.nan), ((2, 1), 3e38)):
            Q = P.copy()
            Q[0][entry] = value
            got, want = shade_both(vis, xy, z, f, c, v, n, Q, K, [(0.3, 0.1, 1.0, 2.0), (0, 0, 0, 8.0)], 0.1, tables[4096], mode)
            assert_shaded(got, want, f"pose entry {entry} = {value}, mode {mode}")


def sr_byte(colours, E, channel):
    """The byte of the plane's centre pixel under linear tables: its colour there is the mean of vertices 0 and 2 (the diagonal)."""
    b = np.floor((float(colours[0, channel]) + float(colours[2, channel])) / 2 + 0.5)
    return int(min(255.0, np.floor(b / 255.0 * E * 255.0 + 0.5)))


# ---------------------------------------------------------------------------------------------- 3. ShadedMeshRenderer
@pytest.fixture(scope="module")
def box_views():
    from gigapose_amd import shade

    v, f, _ = meshes.three_boxes()
    rs = np.random.RandomState(404)
    poses = np.stack([pose(rotation(rs), (rs.uniform(-.2, .2), rs.uniform(-.1, .1), rs.uniform(3.5, 8))) for _ in range(5)]).astype(np.float32)
    lights = shade.blenderproc_lights(1.0)
    out = {}
    for mode in ("smooth", "flat"):
        r = shade.ShadedMeshRenderer(120, 160, K_SMALL / 2 + np.diag([0, 0, 0.5]), ZNEAR, lights, 0.02, shade.srgb_tables(), mode)
        out[mode] = (r, r(_t(v), _t(f), None, _t(poses), colour=(102, 102, 102)))
    return dict(v=v, f=f, poses=poses, lights=lights, out=out, K=(K_SMALL / 2 + np.diag([0, 0, 0.5])).astype(np.float32))


def test_renderer_equals_the_restatement(box_views):
    from gigapose_amd import shade

    s = box_views
    n = sr.vertex_normals(s["v"], s["f"], shade.normal_unit(s["v"]))[2]
    for mode, code in (("smooth", sr.SMOOTH), ("flat", sr.FLAT)):
        got = s["out"][mode][1]
        want = sr.render(s["v"], s["f"], grey(s["v"]), n, s["poses"][:2], s["K"], 120, 160, ZNEAR, s["lights"], 0.02, *shade.srgb_tables(), code)
        assert_bits(got["rgba"][:2], want["rgba"], f"{mode}: rgba")
        assert_bits(got["depth"][:2], want["depth"], f"{mode}: depth")
        assert got["clipped"].tolist() == [0] * 5 and got["unlit"].tolist() == [0] * 5 and (want["rgba"][..., 3] == 255).sum() > 500
        inside = want["rgba"][..., 3] == 255
        assert len(np.unique(want["rgba"][inside][:, 0])) > 10       # shaded: not one flat value


def test_chunking_determinism_and_normals_from_outside(box_views):
    from gigapose_amd import shade

    s = box_views
    args = (_t(s["v"]), _t(s["f"]), None, _t(s["poses"]))
    for mode in ("smooth", "flat"):
        r, base = s["out"][mode]
        again = r(*args, colour=(102, 102, 102))
        chunked = r(*args, colour=(102, 102, 102), views_per_call=2)
        given = r(*args, colour=(102, 102, 102), normals=shade.vertex_normals(args[0], args[1]) * 3.0)      # only the direction counts ... to rounding
        for key in ("rgba", "depth", "clipped", "unlit"):
            assert_bits(again[key], base[key], f"{mode}: {key}, second call")
            assert_bits(chunked[key], base[key], f"{mode}: {key}, two views per call")
        assert_bits(given["depth"], base["depth"], f"{mode}: depth, normals given")
        assert (given["rgba"].int() - base["rgba"].int()).abs().max() <= 1


def test_no_light_and_ambient_one_is_the_mesh_renderer():
    from gigapose_amd import render, shade

    v, f, c = meshes.icosphere(2, 1.0)
    rs = np.random.RandomState(21)
    poses = np.stack([pose(rotation(rs), (0.1, 0.0, d)) for d in (2.0, 5.0, 25.0)] + [pose(np.eye(3), (0, 0, -4.0))]).astype(np.float32)
    args = (_t(v), _t(f), _t(c), _t(poses))
    want = render.MeshRenderer(240, 320, K_SMALL, ZNEAR)(*args, on_clipped="ignore")
    for mode in ("smooth", "flat"):
        r = shade.ShadedMeshRenderer(240, 320, K_SMALL, ZNEAR, None, 1.0, shade.linear_tables(256), mode)
        got = r(*args, on_clipped="ignore")
        for key in ("rgba", "depth", "clipped"):
            assert_bits(got[key], want[key], f"{mode}: {key}")
        assert got["clipped"].tolist() == [0, 0, 0, len(f)] and got["unlit"].tolist() == [0] * 4
        with pytest.raises(ValueError, match=r"view 3 drops 320 of 320 triangles"):
            r(*args)
    assert int((want["rgba"][..., 3] == 255).sum()) > 10000


# ---------------------------------------------------------------------------------------------- 4. addressing past 2^32
def test_views_past_2_to_32_bytes():
    """3 497 views at 480 x 640 in ONE call: rgba is 4.30 GB, so the last view lies past a 32-bit byte offset (and the key buffer
    past 2^33).  Only the last view shows the object and is compared with the restatement; the others look past it."""
    from gigapose_amd import shade

    N, H, W = 3497, 480, 640
    assert (N - 1) * H * W * 4 > 2 ** 32
    v, f, _ = meshes.three_boxes(40.0)
    poses = np.tile(pose(np.eye(3), (50000.0, 0.0, 3000.0)), (N, 1, 1))          # far to the right of the frame, not clipped
    poses[N - 1] = pose(rotation(np.random.RandomState(31)), (-20.0, 12.0, 420.0))
    poses = poses.astype(np.float32)
    lights = shade.blenderproc_lights(100.0)
    r = shade.ShadedMeshRenderer(H, W, syn.TEMPLATE_K, 1e-3, lights, 0.01, shade.srgb_tables(), "smooth")
    out = r(_t(v), _t(f), None, _t(poses), colour=(102, 102, 102), views_per_call=N)
    n = sr.vertex_normals(v, f, shade.normal_unit(v))[2]
    want = sr.render(v, f, grey(v), n, poses[[N - 1]], syn.TEMPLATE_K, H, W, 1e-3, lights, 0.01, *shade.srgb_tables(), sr.SMOOTH)
    assert_bits(out["rgba"][[N - 1]], want["rgba"], "rgba of the last view")
    assert_bits(out["depth"][[N - 1]], want["depth"], "depth of the last view")
    assert int(out["clipped"].abs().sum()) == 0 and int(out["unlit"].abs().sum()) == 0 and (want["rgba"][..., 3] == 255).sum() > 500
    assert int(out["rgba"][N - 2].max()) == 0 and float(out["depth"][1700].abs().max()) == 0.0
    del out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 5. through the model
def test_shaded_templates_through_the_model(tmp_path):
    """three_boxes without colours at 12 views.  Route A: ShadedMeshTemplates (rendered, lit and cropped on the device).  Route B:
    RenderedTemplates on the PNGs save_renders wrote of the same views.  Banks are equal tensor for tensor and so are the
    predictions, in both numerics.  The model is randomly initialised: this proves plumbing, not accuracy."""
    from gigapose_amd import render, shade
    from gigapose_amd.onboard import RenderedTemplates

    v, f, _ = meshes.three_boxes()
    rs = np.random.RandomState(1213)
    poses = np.stack([pose(rotation(rs), (rs.uniform(-.3, .3), rs.uniform(-.2, .2), rs.uniform(4.6, 5.4))) for _ in range(12)]).astype(np.float32)
    mesh_set = shade.ShadedMeshTemplates([((v, f, None), poses)], K=K_SMALL, device=DEV, H=240, W=320, znear=ZNEAR, units_per_metre=1.0,
                                         ambient=0.02, normals="smooth")
    drawn = mesh_set.render(0)
    assert drawn["rgba"].is_cuda and drawn["rgba"].shape == (12, 240, 320, 4) and drawn["unlit"].tolist() == [0] * 12
    inside = drawn["rgba"][..., 3] == 255
    assert int(inside.sum()) > 12 * 1500 and len(torch.unique(drawn["rgba"][inside][:, 0])) > 20      # lit: far from one grey
    assert (drawn["rgba"][inside][:, 0] == drawn["rgba"][inside][:, 2]).all()
    flat = render.MeshTemplates([((v, f, None), poses)], K=K_SMALL, device=DEV, H=240, W=320, znear=ZNEAR, colour=(102, 102, 102)).render(0)
    assert_bits(drawn["depth"], flat["depth"], "depth beside the unshaded renderer")
    assert len(torch.unique(flat["rgba"][inside][:, 0])) == 1
    render.save_renders(tmp_path, drawn["rgba"], drawn["depth"], depth_scale=1000.0)
    png_set = RenderedTemplates([(str(tmp_path), poses)], K=K_SMALL, device=DEV)
    item = mesh_set[0]
    assert item.rgb.is_cuda and item.rgb.shape == (12, 3, 224, 224) and item.mask.shape == (12, 224, 224) and item.poses.shape == (12, 4, 4)
    assert_bits(item.K, K_SMALL, "K")
    model = factory.build_model("dinov2_vits14", k=4, device=DEV, seed=70, numerics="chain")
    syn.condition_ist(model.ist_net)
    tar_K, tar_M = syn.crop_geometry(78, 12)
    labels = torch.ones(12, dtype=torch.int64)
    for numerics in ("chain", "split"):
        model.set_numerics(numerics)
        banks, preds = [], []
        for dataset in (mesh_set, png_set):
            model.template_datasets = {"mesh": dataset}
            model.set_template_data("mesh")
            banks.append({k: t.clone() for k, t in model.template_datas["mesh"].tensors.items()})
            pred = model.predict(item.rgb, item.mask, _t(tar_K), _t(tar_M), labels, "mesh", sort_pred_by_inliers=False)
            torch.cuda.synchronize()
            preds.append({k: getattr(pred, k).clone() for k in ("id_src", "src_pts", "score_src", "pred_poses")})
        assert sorted(banks[0]) == sorted(banks[1]) and len(banks[0]) >= 6
        for key in banks[0]:
            assert_bits(banks[0][key], banks[1][key], f"{numerics}: bank: {key}")
        for key in preds[0]:
            assert_bits(preds[0][key], preds[1][key], f"{numerics}: prediction: {key}")
