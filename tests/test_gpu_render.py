"""GPU: mesh + poses -> RGBA renders and depth (libgigapose_render.so, gigapose_amd/render.py).

The three kernels against the numpy restatement (gigapose_testing/raster_ref.py, written from the header) bit for bit; the
invariance of a polygon's alpha under its triangulation; the conventions (pose, K, pixel centres) and an analytic sphere against
float64 geometry that does not go through the restatement; the real size (162 views at 480 x 640) and a visibility buffer past
2^31 bytes; the error paths; and MeshTemplates -> set_template_data -> predict against RenderedTemplates on the saved PNGs."""
import os

import numpy as np
import pytest
import torch

from gigapose_testing import factory, meshes, raster_ref
from gigapose_testing import synthetic as syn
from gigapose_testing.gpu_cases import DEV, K_SMALL, ZNEAR, assert_bits, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu


def keys(vis):
    return vis.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------------------------------------- 1. gpr_project
def test_project_equals_the_restatement():
    """1 000 random vertices x 5 poses: vertices behind the camera, on the znear plane's two sides, beyond 16384 px, NaN and inf;
    a second call whose projections fall exactly on half a 1/256-pixel step (rint: half to even)."""
    from gigapose_amd import render

    rs = np.random.RandomState(11)
    v = rs.uniform(-1, 1, (1000, 3)).astype(np.float32)
    v[10] = (np.nan, 0, 0)
    v[11] = (0, np.inf, 0)
    v[12] = (0, 0, -np.inf)
    v[13] = (1e30, 0, 0)
    v[14:40, 2] -= 8.0                                              # behind the camera under most poses
    v[40:60, 0] *= 400.0                                            # far to the side: beyond 16384 px at depth ~ 3
    poses = np.stack([pose(rotation(rs), (rs.uniform(-.5, .5), rs.uniform(-.5, .5), rs.uniform(2.5, 4))) for _ in range(5)]).astype(np.float32)
    poses[4] = pose(np.eye(3), (0, 0, 0.5))                         # the vertex cloud straddles the camera plane
    want_xy, want_z = raster_ref.project(v, poses, syn.TEMPLATE_K, ZNEAR)
    bad = want_xy[..., 0] == raster_ref.BAD_COORD
    assert 100 < bad.sum() < 2500 and bad[:, 10:13].all() and bad[4, 13] and not bad[0, 100:].all()   # 1e30 is finite: a rotation can project it
    xy, z = render.project(_t(v), _t(poses), syn.TEMPLATE_K, ZNEAR)
    assert_bits(xy, want_xy, "xy")
    finite = np.isfinite(want_z)
    got_z = z.cpu().numpy()
    assert_bits(got_z[finite], want_z[finite], "depth")
    assert (np.isnan(got_z) == np.isnan(want_z)).all() and (got_z[~finite & ~np.isnan(want_z)] == want_z[~finite & ~np.isnan(want_z)]).all()
    # exact halves: K = 256 px focal, z = 1, x = (2j + 1) / 2^17  ->  u * 256 = j + 1/2 + 32768
    j = np.arange(-300, 300)
    h = np.stack([(2 * j + 1) / 2.0 ** 17, -(2 * j + 1) / 2.0 ** 17, np.ones(len(j))], axis=1).astype(np.float32)
    Kh = np.asarray([256, 0, 128, 0, 256, 128, 0, 0, 1], np.float32)
    eye = np.eye(4, dtype=np.float32)[None]
    want_xy, want_z = raster_ref.project(h, eye, Kh, ZNEAR)
    assert (want_xy[0, :, 0] % 2 == 0).all() and len(np.unique(want_xy[0, :, 0])) == 301       # every tie went to the even side
    xy, z = render.project(_t(h), _t(eye), Kh, ZNEAR)
    assert_bits(xy, want_xy, "xy on exact halves")
    assert_bits(z, want_z, "depth on exact halves")
    # znear is compared with the f32 depth: a vertex exactly on the plane is good, one ulp in front of it is bad
    zn = np.float32(0.25)
    edge = np.asarray([(0, 0, zn), (0, 0, np.nextafter(zn, np.float32(0))), (0, 0, np.nextafter(zn, np.float32(1)))], np.float32)
    xy, _ = render.project(_t(edge), _t(eye), Kh, float(zn))
    assert (xy.cpu().numpy()[0, :, 0] == [128 * 256, raster_ref.BAD_COORD, 128 * 256]).all()


# ---------------------------------------------------------------------------------------------- 2. gpr_raster / gpr_resolve
def factor(pixels, H, W):
    """(w, h) with w * h == pixels that fits the frame with a margin, or None."""
    for h in range(2, H - 4):
        if pixels % h == 0 and pixels // h <= W - 4:
            return pixels // h, h
    return None


def right_triangle(x0, y0, w, h):
    """Screen vertices of a right triangle whose clamped bounding box is exactly w x h pixels (corners on pixel centres)."""
    return [(x0 * 256, y0 * 256), ((x0 + w - 1) * 256, y0 * 256), (x0 * 256, (y0 + h - 1) * 256)]


def scenes(H, W):
    """name -> (xy (V,2) int32, depth (V,) f32, faces (F,3) int32, colours (V,3) u8): one view each."""
    from gigapose_amd import render

    rs = np.random.RandomState(H * 7 + W)
    T = render.small_triangle_pixels()
    out = {}
    # the fan polygons of tests/test_render_host.py, as hand-made screen coordinates with a depth of their own per vertex
    for k in range(6):
        p, c = meshes.screen_polygon(rs, H, W, on_centres=k % 2 == 0)
        for about_centre in (False, True):
            xy = np.concatenate([p, c]).astype(np.int32)
            faces = meshes.fan_faces(len(p), about_centre)
            if k % 3 == 2:
                faces = faces[:, ::-1].copy()                        # the other winding
            out[f"polygon {k} ({len(p)} vertices), fan about {'the centre' if about_centre else 'vertex 0'}"] = (
                xy, rs.uniform(1, 3, len(xy)).astype(np.float32), faces, rs.randint(0, 256, (len(xy), 3)).astype(np.uint8))
    # a box whose 12 faces straddle the small / large threshold + triangles at threshold - 1, threshold, threshold + 1 pixels
    v, f, c = meshes.box((1.0, 0.6, 0.15))
    K = np.asarray([W * 0.9, 0, (W - 1) / 2, 0, W * 0.9, (H - 1) / 2, 0, 0, 1], np.float32)
    R = rotation(np.random.RandomState(3))
    xy, z = raster_ref.project(v, pose(R, (0.0, 0.0, 1.6))[None].astype(np.float32), K, ZNEAR)
    xy, z = xy[0], z[0]
    sizes = [raster_ref.box_pixels(xy, f, i, H, W) for i in range(len(f))]
    assert min(sizes) <= T < max(sizes), f"the box faces do not straddle {T}: {sizes}"
    extra_xy, extra_f, extra_c, extra_z = [], [], [], []
    for i, pixels in enumerate((T - 1, T, T + 1)):
        wh = factor(pixels, H, W)
        assert wh is not None, f"{pixels} pixels do not factor into a box inside {W} x {H}"
        tri = right_triangle(1 + i, 2 + i, *wh)
        extra_f.append([len(v) + len(extra_xy) + j for j in range(3)])
        extra_xy += tri
        extra_c += [(60 * i + 20, 255 - 50 * i, 90)] * 3
        extra_z += [0.9 + 0.3 * i, 2.5, 1.4]                        # they cut through the box and through one another
    bxy = np.concatenate([xy, np.asarray(extra_xy, np.int32)]).astype(np.int32)
    bf = np.concatenate([f, np.asarray(extra_f, np.int32)]).astype(np.int32)
    got = [raster_ref.box_pixels(bxy, bf, len(f) + i, H, W) for i in range(3)]
    assert got == [T - 1, T, T + 1], got
    out["box across the threshold"] = (bxy, np.concatenate([z, np.asarray(extra_z, np.float32)]), bf, np.concatenate([c, np.asarray(extra_c, np.uint8)]))
    # special triangles in one view
    big = [(-5 * W * 256 + 37, -4 * H * 256 + 11), (6 * W * 256 + 5, -5 * H * 256), (W * 128 + 77, H * 230 + 3)]           # ten times the frame, apex inside
    outside = [((W + 3) * 256, 5 * 256), ((W + 40) * 256, 9 * 256), ((W + 9) * 256, (H + 30) * 256)]
    line = [(2 * 256, 2 * 256), (12 * 256, 7 * 256), (22 * 256, 12 * 256)]                                                  # zero area
    dup = [(5 * 256 + 128, 4 * 256 + 3), ((W - 6) * 256, 9 * 256 + 200), (W * 100, (H - 3) * 256 + 9)]
    badv = [(0, 0), (10 * 256, 0), (int(raster_ref.BAD_COORD), int(raster_ref.BAD_COORD))]
    pts = big + outside + line + dup + dup + badv
    depth = [9.0, 7.0, 8.0] + [1.0] * 3 + [1.0] * 3 + [2.0, 3.0, 5.0] * 2 + [1.0, 1.0, -4.0]
    colours = [(200, 10, 10), (10, 200, 10), (10, 10, 200)] + [(255, 255, 255)] * 6 + [(250, 240, 0)] * 3 + [(0, 240, 250)] * 3 + [(9, 9, 9)] * 3
    faces = [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(6)] + [(0, 1, 18), (0, -1, 2)]                                    # + indices outside the mesh
    out["special triangles"] = (np.asarray(pts, np.int32), np.asarray(depth, np.float32), np.asarray(faces, np.int32), np.asarray(colours, np.uint8))
    return out, T


@pytest.fixture(scope="module", params=[(48, 64), (120, 160)], ids=["64x48", "160x120"])
def drawn(request):
    """Every scene drawn once by the kernels and once by the restatement."""
    from gigapose_amd import render

    H, W = request.param
    all_scenes, T = scenes(H, W)
    res = {}
    for name, (xy, z, faces, colours) in all_scenes.items():
        d_xy, d_z, d_f, d_c = _t(xy[None]), _t(z[None]), _t(faces), _t(colours)
        vis, clipped = render.raster(d_xy, d_z, d_f, H, W)
        rgba, depth = render.resolve(vis, d_xy, d_z, d_f, d_c)
        want_vis, want_clipped = raster_ref.raster(xy[None], z[None], faces, H, W)
        want_rgba, want_depth = raster_ref.resolve(want_vis, xy[None], z[None], faces, colours)
        res[name] = dict(scene=(xy, z, faces, colours), got=(keys(vis), clipped.cpu().numpy(), rgba.cpu().numpy(), depth.cpu().numpy()),
                         want=(want_vis, want_clipped, want_rgba, want_depth))
    return dict(H=H, W=W, T=T, res=res)


def test_raster_keys_equal_the_restatement(drawn):
    for name, r in drawn["res"].items():
        assert_bits(r["got"][0], r["want"][0], f"keys of '{name}'")
        assert_bits(r["got"][1], r["want"][1], f"clipped of '{name}'")
        covered = r["want"][0] != raster_ref.EMPTY_KEY
        assert covered.any() and not covered.all(), name


def test_resolve_equals_the_restatement(drawn):
    for name, r in drawn["res"].items():
        assert_bits(r["got"][2], r["want"][2], f"rgba of '{name}'")
        assert_bits(r["got"][3], r["want"][3], f"depth of '{name}'")
        a = r["got"][2][..., 3]
        assert set(np.unique(a)) == {0, 255}
        assert (r["got"][3][a == 0] == 0).all() and (r["got"][3][a == 255] > 0).all()
        assert (r["got"][2][a == 0] == 0).all()


def test_both_launch_paths_write_one_image(drawn):
    """The box scene: faces at or below the threshold are walked by one thread, the others by a workgroup; each path owns pixels
    of the final image, and so does each of the triangles at threshold - 1, threshold and threshold + 1 pixels."""
    H, W, T = drawn["H"], drawn["W"], drawn["T"]
    r = drawn["res"]["box across the threshold"]
    xy, _, faces, _ = r["scene"]
    owner = (r["got"][0] & np.uint64(0xFFFFFFFF)).astype(np.int64)[r["got"][0] != raster_ref.EMPTY_KEY]
    sizes = np.asarray([raster_ref.box_pixels(xy, faces, f, H, W) for f in range(len(faces))])
    owners = set(np.unique(owner).tolist())
    assert any(sizes[f] <= T for f in owners) and any(sizes[f] > T for f in owners)
    assert {len(faces) - 3, len(faces) - 2, len(faces) - 1} <= owners


def test_special_triangles(drawn):
    H, W = drawn["H"], drawn["W"]
    r = drawn["res"]["special triangles"]
    vis, clipped, rgba, depth = r["got"]
    assert clipped.tolist() == [3]                                  # the bad vertex and the two faces with an index outside the mesh
    face = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    covered = vis != raster_ref.EMPTY_KEY
    assert set(np.unique(face[covered])) == {0, 3}                  # outside, zero area, the higher duplicate and the clipped ones own nothing
    assert covered.sum() > 0.5 * H * W and (face[covered] == 0).sum() > 0.2 * H * W       # the triangle ten times the frame
    assert (rgba[0][face[0] == 3][:, :3] == (250, 240, 0)).all() and (face == 3).sum() > 20   # the lower face index wins


def test_reversed_face_list_gives_the_same_depths(drawn):
    from gigapose_amd import render

    H, W = drawn["H"], drawn["W"]
    for name in ("box across the threshold", "special triangles"):
        r = drawn["res"][name]
        xy, z, faces, colours = r["scene"]
        vis, clipped = render.raster(_t(xy[None]), _t(z[None]), _t(faces[::-1].copy()), H, W)
        assert_bits(keys(vis) >> np.uint64(32), r["got"][0] >> np.uint64(32), f"depth bits of '{name}' reversed")
        _, depth = render.resolve(vis, _t(xy[None]), _t(z[None]), _t(faces[::-1].copy()), _t(colours))
        assert_bits(depth, r["got"][3], f"depth of '{name}' reversed")
        assert clipped.tolist() == r["got"][1].tolist()


# ---------------------------------------------------------------------------------------------- 3. tessellation invariance
def test_alpha_of_a_convex_polygon_does_not_depend_on_its_triangulation():
    """200 seeded polygons as the 200 views of one launch (padded to 8 vertices + the interior point): fan about vertex 0, fan
    about the interior point, and both with the other winding give the same alpha, which is the restatement's."""
    from gigapose_amd import render

    H, W, N = 48, 64, 200
    rs = np.random.RandomState(77)
    polys = [meshes.screen_polygon(rs, H, W, on_centres=k % 2 == 0) for k in range(N)]
    xy = np.stack([meshes.padded_polygon(p, c) for p, c in polys])
    z = np.ones(xy.shape[:2], np.float32)
    alphas = []
    for about_centre in (False, True):
        for flip in (False, True):
            faces = meshes.fan_faces(meshes.MAX_POLY, about_centre)
            faces = faces[:, ::-1].copy() if flip else faces
            vis, clipped = render.raster(_t(xy), _t(z), _t(faces), H, W)
            assert int(clipped.abs().sum()) == 0
            alphas.append(keys(vis) != raster_ref.EMPTY_KEY)
    for a in alphas[1:]:
        assert (a == alphas[0]).all(), f"{int((a != alphas[0]).any(axis=(1, 2)).sum())} polygons differ"
    want = np.stack([raster_ref.coverage(np.concatenate([p, c]), meshes.fan_faces(len(p), False), H, W) for p, c in polys])
    assert want.max() == 1 and (alphas[0] == (want == 1)).all()
    assert alphas[0].reshape(N, -1).sum(axis=1).mean() > 200         # slivers that hold a few pixels or none are among them, not the rule


# ---------------------------------------------------------------------------------------------- 4. conventions, against float64
def ray_hits(origin_dirs, tris):
    """Moeller-Trumbore in float64: rays from the origin along (R,3) directions against (T,3,3) triangles -> t (R,T), inf = miss."""
    a, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    d = origin_dirs[:, None, :]
    p = np.cross(d, e2[None])
    det = (p * e1[None]).sum(-1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        s = -a[None]
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1[None])
        v = (d * q).sum(-1) * inv
        t = (e2[None] * q).sum(-1) * inv
    hit = (np.abs(det) > 1e-14) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return np.where(hit, t, np.inf)


def draw_three_boxes():
    from gigapose_amd import render

    v, f, c = meshes.three_boxes()
    rs = np.random.RandomState(404)
    poses = np.stack([pose(rotation(rs), (rs.uniform(-.6, .6), rs.uniform(-.4, .4), rs.uniform(4.5, 6))) for _ in range(5)])
    out = render.MeshRenderer(240, 320, K_SMALL, ZNEAR)(_t(v), _t(f), _t(c), _t(poses.astype(np.float32)))
    return dict(v=v, f=f, c=c, poses=poses.astype(np.float32).astype(np.float64), out=out)


@pytest.fixture(scope="module")
def three_boxes_views():
    return draw_three_boxes()


def test_conventions_against_float64(three_boxes_views):
    """The asymmetric three-box object under 5 seeded poses, checked against K [R|t] in float64 (not the restatement).  For every
    quad, the pixel p nearest the projection of its centroid: when the float64 rays through p and through p +- 1/4 pixel all hit
    this quad first (so that neither the 1/256-pixel snap of the vertices nor an occluder's rim can decide), p carries the quad's
    colour and the depth of the float64 hit to 1e-4 relative.  The alpha box is the box of the projected vertices to +- 1 px.
    A transposed rotation, a y-up camera or a half-pixel shift fail all three."""
    from gigapose_amd import onboard

    s = three_boxes_views
    v, f, c = s["v"].astype(np.float64), s["f"], s["c"]
    K = K_SMALL.astype(np.float64)
    Kinv = np.linalg.inv(K)
    rgba, depth = s["out"]["rgba"].cpu().numpy(), s["out"]["depth"].cpu().numpy()
    boxes = onboard.alpha_boxes(s["out"]["rgba"]).cpu().numpy()
    assert s["out"]["clipped"].tolist() == [0] * 5
    checked = 0
    for n, P in enumerate(s["poses"]):
        cam = v @ P[:3, :3].T + P[:3, 3]
        uv = cam @ K.T
        uv = uv[:, :2] / uv[:, 2:]
        tris = cam[f]                                               # (F,3,3)
        quad_of = np.arange(len(f)) // 2
        for quad in range(len(f) // 2):
            corners = np.unique(f[2 * quad:2 * quad + 2])
            centre = cam[corners].mean(axis=0)
            pc = K @ centre
            px, py = int(np.rint(pc[0] / pc[2])), int(np.rint(pc[1] / pc[2]))
            if not (1 <= px < 319 and 1 <= py < 239):
                continue
            probes = np.asarray([(px + dx, py + dy, 1.0) for dx, dy in ((0, 0), (.25, .25), (-.25, .25), (.25, -.25), (-.25, -.25))])
            t = ray_hits(probes @ Kinv.T, tris)                     # directions with z = 1: t is the camera depth of the hit
            first = t.argmin(axis=1)
            if not (np.isfinite(t.min(axis=1)).all() and (quad_of[first] == quad).all()):
                continue                                            # hidden, or too near an edge to be decided by float64 alone
            checked += 1
            colour = c[corners[0]]
            assert rgba[n, py, px].tolist() == colour.tolist() + [255], f"view {n}, quad {quad}, pixel ({px}, {py})"
            z = t[0].min()
            print(f"view {n} quad {quad}: depth {depth[n, py, px]:.6f} float64 {z:.6f} rel {abs(depth[n, py, px] - z) / z:.2e}")
            assert abs(depth[n, py, px] - z) <= 1e-4 * z, f"view {n}, quad {quad}: depth {depth[n, py, px]} vs {z}"
        want = [np.ceil(uv[:, 0].min()), np.ceil(uv[:, 1].min()), np.floor(uv[:, 0].max()) + 1, np.floor(uv[:, 1].max()) + 1]
        print(f"view {n}: alpha box {boxes[n].tolist()} float64 {want}")
        assert np.abs(boxes[n] - np.asarray(want)).max() <= 1, f"view {n}: alpha box {boxes[n].tolist()} vs {want}"
    assert checked >= 25, f"only {checked} quads were decidable"


# ---------------------------------------------------------------------------------------------- 5. analytic sphere
def sphere_extent(c0, cz, r, focal, centre):
    """The two image coordinates (one axis) of the planes through the camera's other axis that touch a sphere at (c0, cz) of
    radius r: |c0 - u cz| / sqrt(1 + u^2) = r  ->  u^2 (cz^2 - r^2) - 2 c0 cz u + (c0^2 - r^2) = 0."""
    a, b, c = cz * cz - r * r, -2 * c0 * cz, c0 * c0 - r * r
    disc = np.sqrt(b * b - 4 * a * c)
    return focal * (-b - disc) / (2 * a) + centre, focal * (-b + disc) / (2 * a) + centre


def ray_sphere_depth(direction, centre, r):
    """Camera depth of the first hit of the ray t * direction (direction z = 1) with the sphere."""
    a, b, c = direction @ direction, -2 * direction @ centre, centre @ centre - r * r
    return (-b - np.sqrt(b * b - 4 * a * c)) / (2 * a)


@pytest.mark.parametrize("centre", [(0.0, 0.0, 6.0), (1.7, -1.1, 6.5)], ids=["on axis", "off axis"])
def test_icosphere_against_the_analytic_sphere(centre):
    """An icosphere of 1 280 faces with its vertices ON the sphere of radius r is convex and holds the origin, so it lies between
    that sphere and the sphere of radius r_in = the least distance of a face's plane from the centre.  With n = pi / (the largest
    angle between a face's nearest point and its vertices) that is r_in = r cos(pi / n): the faceting bound r (1 - cos(pi / n)).
    Hence every edge of the alpha box lies between the analytic extents of the two spheres (+- 1 px for the sampling), and the
    depth along the ray of the pixel at the projected centre between the two spheres' hits."""
    from gigapose_amd import onboard, render

    r = 1.0
    v, f, c = meshes.icosphere(3, r)
    assert len(f) == 1280
    tri = v.astype(np.float64)[f]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    r_in = np.abs((normal * tri[:, 0]).sum(-1)).min()
    n_eff = np.pi / np.arccos(r_in / r)
    assert 0.98 * r < r_in < r and abs(r * (1 - np.cos(np.pi / n_eff)) - (r - r_in)) < 1e-12
    centre = np.asarray(centre)
    P = pose(rotation(np.random.RandomState(8)), centre).astype(np.float32)
    out = render.MeshRenderer(240, 320, K_SMALL, ZNEAR)(_t(v), _t(f), _t(c), _t(P[None]))
    box = onboard.alpha_boxes(out["rgba"]).cpu().numpy()[0]
    K = K_SMALL.astype(np.float64)
    for axis, (lo, hi) in enumerate(((box[0], box[2] - 1), (box[1], box[3] - 1))):
        outer = sphere_extent(centre[axis], centre[2], r, K[axis, axis], K[axis, 2])
        inner = sphere_extent(centre[axis], centre[2], r_in, K[axis, axis], K[axis, 2])
        print(f"axis {axis}: alpha {lo}..{hi}, sphere {outer[0]:.3f}..{outer[1]:.3f}, inscribed {inner[0]:.3f}..{inner[1]:.3f}")
        assert outer[0] - 1 <= lo <= inner[0] + 1 and inner[1] - 1 <= hi <= outer[1] + 1
        assert inner[0] - outer[0] < 1.0                             # the faceting bound is below one pixel here: the check is tight
    pc = K @ centre
    px, py = int(np.rint(pc[0] / pc[2])), int(np.rint(pc[1] / pc[2]))
    d = np.linalg.inv(K) @ np.asarray([px, py, 1.0])
    near, far = ray_sphere_depth(d, centre, r), ray_sphere_depth(d, centre, r_in)
    got = float(out["depth"][0, py, px])
    print(f"centre pixel ({px}, {py}): depth {got:.6f}, sphere {near:.6f}, inscribed {far:.6f}")
    assert near * (1 - 1e-6) <= got <= far * (1 + 1e-6)
    if centre[0] == 0:
        assert abs(near - (centre[2] - r)) < 1e-12                   # on axis the ray goes through the centre: d - r


# ---------------------------------------------------------------------------------------------- 6. real size
def draw_level1(golden_dir, views=None):
    """162 views at 480 x 640: an icosphere of 320 faces and radius r, the camera 4 r away (the reference's 0.4 x 1000 mm for an
    object of 100 mm radius)."""
    from gigapose_amd import render

    r = 35.0
    v, f, c = meshes.icosphere(2, r)
    v = (v * np.asarray([1.0, 0.8, 0.6], np.float32)).astype(np.float32)     # not a sphere: every view differs
    poses = np.load(os.path.join(golden_dir, "template_poses_level1.npy"))
    assert poses.shape == (162, 4, 4)
    poses = render.template_object_poses(poses)
    poses[:, :3, 3] *= r / 100.0
    poses = poses.astype(np.float32)
    out = render.MeshRenderer()(_t(v), _t(f), _t(c), _t(poses if views is None else poses[views]), views_per_call=162)
    return dict(v=v, f=f, c=c, poses=poses, out=out)


@pytest.fixture(scope="module")
def level1_views(golden_dir):
    return draw_level1(golden_dir)


def test_real_size_162_views(level1_views):
    """No view is clipped, every alpha box is inside the frame, views 0 and 161 equal the restatement bit for bit.  (The
    visibility buffer of 162 views is 398 MB: the offsets past 2^31 bytes are test_views_past_2_to_31_bytes's.)"""
    from gigapose_amd import onboard

    s = level1_views
    out = s["out"]
    assert out["rgba"].shape == (162, 480, 640, 4) and out["depth"].shape == (162, 480, 640)
    assert int(out["clipped"].abs().sum()) == 0
    boxes = onboard.alpha_boxes(out["rgba"]).cpu().numpy()
    assert (boxes[:, :2] > 0).all() and (boxes[:, 2] < 640).all() and (boxes[:, 3] < 480).all()
    assert ((boxes[:, 2] - boxes[:, 0]) > 100).all()
    pick = [0, 161]
    want = raster_ref.render(s["v"], s["f"], s["c"], s["poses"][pick], syn.TEMPLATE_K, 480, 640, 1e-3)
    assert_bits(out["rgba"][pick], want["rgba"], "rgba of views 0 and 161")
    assert_bits(out["depth"][pick], want["depth"], "depth of views 0 and 161")
    assert not (want["rgba"][0] == want["rgba"][1]).all()


def test_views_past_2_to_31_bytes():
    """900 views at 480 x 640 in ONE call: the visibility buffer is 2.2 GB, view 874 onwards lies past a 32-bit byte offset in it
    (and view 1748 / 2 = 874 likewise in the depth output's 1.1 GB... the rgba and depth outputs stay below 2^31).  All views
    share one pose except the last, which must equal the restatement bit for bit, as must the first."""
    from gigapose_amd import render

    N, H, W = 900, 480, 640
    assert N * H * W * 8 > 2 ** 31
    v, f, c = meshes.three_boxes(40.0)
    rs = np.random.RandomState(31)
    poses = np.tile(pose(rotation(rs), (5.0, -3.0, 260.0)), (N, 1, 1))
    poses[N - 1] = pose(rotation(rs), (-20.0, 12.0, 230.0))
    poses = poses.astype(np.float32)
    out = render.MeshRenderer()(_t(v), _t(f), _t(c), _t(poses), views_per_call=N)
    want = raster_ref.render(v, f, c, poses[[0, N - 1]], syn.TEMPLATE_K, H, W, 1e-3)
    assert_bits(out["rgba"][[0, N - 1]], want["rgba"], "rgba of the first and the last view")
    assert_bits(out["depth"][[0, N - 1]], want["depth"], "depth of the first and the last view")
    assert_bits(out["rgba"][N - 2], want["rgba"][0], "rgba of the view before the last")
    assert int(out["clipped"].abs().sum()) == 0 and (want["rgba"][..., 3] == 255).sum() > 5000
    del out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 7. errors, determinism
def test_error_behaviour():
    from gigapose_amd import _lib, render

    v, f, c = meshes.three_boxes()
    good = pose(np.eye(3), (0, 0, 5.0))
    behind = pose(np.eye(3), (0, 0, -5.0))
    poses = np.stack([good, good, behind, good]).astype(np.float32)
    r = render.MeshRenderer(48, 64, K_SMALL / 5 + np.diag([0, 0, 0.8]).astype(np.float32), ZNEAR)
    dv, df, dc, dp = _t(v), _t(f), _t(c), _t(poses)
    with pytest.raises(ValueError, match=r"view 2 drops 48 of 48 triangles"):
        r(dv, df, dc, dp)
    out = r(dv, df, dc, dp, on_clipped="ignore")
    assert out["clipped"].tolist() == [0, 0, len(f), 0]
    assert int(out["rgba"][2].max()) == 0 and int(out["rgba"][0, ..., 3].max()) == 255
    for args in ((dv.cpu(), df, dc, dp), (dv, df.cpu(), dc, dp), (dv, df, dc.cpu(), dp), (dv, df, dc, dp.cpu()), (v, f, c, poses)):
        with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
            r(*args)
    with pytest.raises(ValueError, match="textures are out of scope"):
        r(dv, df, None, dp[:1])
    grey = r(dv, df, None, dp[:1], colour=(102, 102, 102))
    a = grey["rgba"][0]
    assert (a[a[..., 3] == 255][:, :3] == 102).all() and int((a[..., 3] == 255).sum()) > 50
    assert_bits(grey["rgba"][..., 3], out["rgba"][:1, ..., 3], "alpha does not depend on the colours")


def test_two_runs_give_the_same_bits(three_boxes_views):
    from gigapose_amd import render

    s = three_boxes_views
    again = render.MeshRenderer(240, 320, K_SMALL, ZNEAR)(_t(s["v"]), _t(s["f"]), _t(s["c"]), _t(s["poses"].astype(np.float32)))
    for key in ("rgba", "depth", "clipped"):
        assert_bits(again[key], s["out"][key], key)
    chunked = render.MeshRenderer(240, 320, K_SMALL, ZNEAR)(_t(s["v"]), _t(s["f"]), _t(s["c"]), _t(s["poses"].astype(np.float32)), views_per_call=2)
    for key in ("rgba", "depth", "clipped"):
        assert_bits(chunked[key], s["out"][key], f"{key}, two views per call")


# ---------------------------------------------------------------------------------------------- 8. through the model
@pytest.fixture(scope="module")
def vits_model():
    model = factory.build_model("dinov2_vits14", k=4, device=DEV, seed=70, numerics="chain")
    syn.condition_ist(model.ist_net)
    return model


def test_mesh_templates_through_the_model(vits_model, tmp_path):
    """The three-box object at 12 seeded views.  Route A: MeshTemplates (rendered and cropped on the device).  Route B:
    RenderedTemplates on the PNGs save_renders wrote of the same views.  Banks are equal tensor for tensor; with every
    template's own crop and mask as the query, predict returns that template first, in both numerics."""
    from gigapose_amd import render
    from gigapose_amd.onboard import RenderedTemplates

    v, f, c = meshes.three_boxes()
    rs = np.random.RandomState(1212)
    poses = np.stack([pose(rotation(rs), (rs.uniform(-.3, .3), rs.uniform(-.2, .2), rs.uniform(4.6, 5.4))) for _ in range(12)]).astype(np.float32)
    mesh_set = render.MeshTemplates([((v, f, c), poses)], K=K_SMALL, device=DEV, H=240, W=320, znear=ZNEAR)
    drawn = mesh_set.render(0)
    assert drawn["rgba"].is_cuda and drawn["rgba"].shape == (12, 240, 320, 4)
    render.save_renders(tmp_path, drawn["rgba"], drawn["depth"], depth_scale=1000.0)
    png_set = RenderedTemplates([(str(tmp_path), poses)], K=K_SMALL, device=DEV)
    item = mesh_set[0]
    assert item.rgb.is_cuda and item.rgb.shape == (12, 3, 224, 224) and item.mask.shape == (12, 224, 224) and item.poses.shape == (12, 4, 4)
    assert_bits(item.K, K_SMALL, "K")
    assert set(torch.unique(item.mask).tolist()) == {0.0, 1.0}
    tar_K, tar_M = syn.crop_geometry(78, 12)
    labels = torch.ones(12, dtype=torch.int64)
    model = vits_model
    for numerics in ("chain", "split"):
        model.set_numerics(numerics)
        banks = []
        for dataset in (mesh_set, png_set):
            model.template_datasets = {"mesh": dataset}
            model.set_template_data("mesh")
            banks.append({k: t.clone() for k, t in model.template_datas["mesh"].tensors.items()})
        assert sorted(banks[0]) == sorted(banks[1]) and len(banks[0]) >= 6
        for key in banks[0]:
            assert_bits(banks[0][key], banks[1][key], f"{numerics} bank: {key}")
        pred = model.predict(item.rgb, item.mask, _t(tar_K), _t(tar_M), labels, "mesh", sort_pred_by_inliers=False)
        torch.cuda.synchronize()
        assert pred.id_src[:, 0].cpu().tolist() == list(range(12)), f"{numerics}: {pred.id_src[:, 0].cpu().tolist()}"
