"""CPU: the restatement of libgigapose_shade.so (gigapose_testing/shade_ref.py, written from include/gigapose_shade.h) on trial, and
the host side of gigapose_amd/shade.py.

Vertex normals against Python integers and fractions.Fraction; the pixel arithmetic against closed forms (a plane under one light,
a sphere lit from the camera's centre); invariances (winding, a light behind the surface, no light at all = the unshaded
resolve, a rigid motion of object and lights together); what the shading is FOR (a grey box stops being one flat value);
and seven subtly wrong shaders, each rejected by the check named beside it.  tests/test_gpu_shade.py holds the kernels to this
restatement bit for bit."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from gigapose_amd import _lib, shade
from gigapose_testing import meshes, raster_ref
from gigapose_testing import shade_ref as sr
from gigapose_testing.symbols import exported_symbols

ZNEAR = 1e-3
EPS = 2.0 ** -53


def pose(R=np.eye(3), t=(0.0, 0.0, 0.0)):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P.astype(np.float32)


def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def centred_K(H, W, focal):
    return np.asarray([[focal, 0, (W - 1) / 2], [0, focal, (H - 1) / 2], [0, 0, 1]], np.float32)


def grey(v, value=102):
    return np.full((len(v), 3), value, np.uint8)


def int_cross(p0, p1, p2):
    u, w = [int(b) - int(a) for a, b in zip(p0, p1)], [int(b) - int(a) for a, b in zip(p0, p2)]
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def int_acc(v, f, unit):
    acc = [[0, 0, 0] for _ in v]
    for face in f:
        c = int_cross(*(v[i] for i in face))
        for i in face:
            for k in range(3):
                acc[i][k] += c[k] * unit
    return acc


def shared_cube():
    corners = np.asarray([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float32)
    f = [t for quad, _ in meshes._BOX_FACES for t in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3]))]
    return corners, np.asarray(f, np.int32)


def octahedron():
    v = np.asarray([(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)], np.float32)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.asarray(f, np.int32)


# ---------------------------------------------------------------------------------------------- the library and its header
def test_shade_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_shade.so", "gpl")         # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_shade.h" and side.path == shade.SHADE_LIB_PATH
    assert sorted(protos) == ["gpl_abi_version", "gpl_last_error", "gpl_shade", "gpl_vertex_normals"]
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpl_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_", "gpf_", "gpv_", "gpm_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the shade library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert lib.gpl_vertex_normals.argtypes == [P, I, P, I, D, P, P, P, P]
    assert lib.gpl_shade.argtypes == [P, P, P, I, P, I, P, P, P, P, P, P, I, D, P, P, I, I, I, I, I, P, P, P, P]
    assert lib.gpl_abi_version() == 1
    text = open(_lib.INCLUDE_DIR + "/gigapose_shade.h").read()
    for name, value in (("GPL_RANGE", sr.RANGE), ("GPL_NO_NORMAL", sr.NO_NORMAL), ("GPL_SMOOTH", sr.SMOOTH), ("GPL_FLAT", sr.FLAT),
                        ("GPL_MAX_LIGHTS", sr.MAX_LIGHTS)):
        assert f"#define {name} {value}" in text and getattr(shade, name[4:]) == value


def test_argument_validation_needs_no_gpu():
    """Every refusal is decided on the host before a launch: -1 and a message."""
    lib = _lib.SideLibrary("libgigapose_shade.so", "gpl").lib()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    p = P(4096)
    K = (ctypes.c_float * 9)(100, 0, 10, 0, 100, 10, 0, 0, 1)
    K0 = (ctypes.c_float * 9)(0, 0, 10, 0, 100, 10, 0, 0, 1)
    lights = (ctypes.c_double * 68)()

    def normals(V=3, F=1, unit=1.0, acc=p, vertices=p):
        return lib.gpl_vertex_normals(vertices, I(V), p, I(F), D(unit), acc, p, p, P(0))

    def shaded(L=1, T=256, mode=0, N=1, K=K, rgba=p, normals=p, lights=lights, H=4):
        return lib.gpl_shade(p, p, p, I(3), p, I(1), p, p, normals, p, K, lights, I(L), D(0.0), p, p, I(T), I(mode), I(N), I(H), I(4), rgba, p, p, P(0))

    for refuse, word in ((lambda: normals(V=0), "bad sizes"), (lambda: normals(F=-1), "bad sizes"), (lambda: normals(unit=0.0), "unit"), (lambda: normals(unit=math.inf), "unit"),
                     (lambda: normals(unit=math.nan), "unit"), (lambda: normals(acc=P(0)), "null"), (lambda: normals(acc=P(4100)), "aligned"), (lambda: normals(vertices=P(0)), "null"),
                     (lambda: shaded(L=17), "lights"), (lambda: shaded(L=-1), "lights"), (lambda: shaded(T=255), "table"), (lambda: shaded(T=65537), "table"), (lambda: shaded(mode=2), "mode"),
                     (lambda: shaded(N=65536), "bad sizes"), (lambda: shaded(H=0), "bad sizes"), (lambda: shaded(K=K0), "K[0]"), (lambda: shaded(rgba=P(4098)), "4-byte"),
                     (lambda: shaded(normals=P(0)), "null"), (lambda: shaded(lights=P(0)), "null"), (lambda: shaded(K=P(0)), "null")):
        rc = refuse()
        assert rc == -1 and word in lib.gpl_last_error().decode(), (rc, word, lib.gpl_last_error().decode())
    assert shaded(N=0) == 0


# ---------------------------------------------------------------------------------------------- 1. vertex normals
def test_accumulated_integers_equal_python_integers():
    rs = np.random.RandomState(7)
    for V, F in ((4, 3), (9, 40), (30, 200)):
        v = rs.randint(-9, 10, (V, 3)).astype(np.float32)
        f = rs.randint(0, V, (F, 3)).astype(np.int32)                # degenerate and repeated corners included
        acc, flags, n = sr.vertex_normals(v, f, 4.0)
        assert acc.tolist() == int_acc(v, f, 4)
        assert ((flags == sr.NO_NORMAL) == (acc == 0).all(axis=1)).all() and not (flags & sr.RANGE).any()
        assert ((n == 0).all(axis=1) == (flags != 0)).all()


def check_cube_and_octahedron(wrong=None):
    """The direction is the exact integer sum; each component agrees with the Fraction a_k^2 / (a . a) to the two roundings of
    the root and the quotient; an octahedron's normals are its axes exactly."""
    for v, f in (shared_cube(), octahedron()):
        acc, flags, n = sr.vertex_normals(v, f, 8.0, wrong=wrong)
        want = int_acc(v, f, 8)
        assert acc.tolist() == want and not flags.any()
        for a, got in zip(want, n):
            aa = sum(k * k for k in a)
            for k in range(3):
                assert np.sign(got[k]) == np.sign(a[k])
                g2 = Fraction(float(got[k])) ** 2
                assert abs(g2 - Fraction(a[k] * a[k], aa)) <= Fraction(a[k] * a[k], aa) * Fraction(6, 2 ** 53), (a, got)
    v, f = octahedron()
    n = sr.vertex_normals(v, f, 1.0, wrong=wrong)[2]
    assert n.tolist() == (v / 2).tolist()
    corner = sr.vertex_normals(*shared_cube(), 1.0, wrong=wrong)[2]
    assert len({tuple(np.abs(c)) for c in corner.tolist()}) > 1       # area weights: the triangulation shows in a cube's corners


def test_cube_and_octahedron_normals_are_fraction_directions():
    check_cube_and_octahedron()


def test_normals_do_not_depend_on_the_order_of_faces_or_corners():
    rs = np.random.RandomState(3)
    v, f, _ = meshes.icosphere(2, 0.7)
    v = (v + rs.normal(scale=0.01, size=v.shape)).astype(np.float32)
    unit = shade.normal_unit(v)
    base = sr.vertex_normals(v, f, unit)
    assert not base[1].any() and np.abs(np.linalg.norm(base[2], axis=1) - 1).max() < 4 * EPS
    g = f[rs.permutation(len(f))]
    g = np.stack([np.roll(row, rs.randint(3)) for row in g]).astype(np.int32)
    for a, b in zip(base, sr.vertex_normals(v, g, unit)):
        assert a.tobytes() == b.tobytes()
    flipped = sr.vertex_normals(v, f[:, [0, 2, 1]], unit)
    assert (flipped[0] == -base[0]).all() and (flipped[2] == -base[2]).all()


def test_a_fan_of_70_triangles_is_summed_correctly():
    v, f = sr.fan(70)
    acc, flags, n = sr.vertex_normals(v, f, 2.0)
    assert acc.tolist() == int_acc(v, f, 2) and not flags.any()
    assert acc[0, 2] > 0 and abs(n[0, 2] - 1) < 1e-3


@pytest.mark.parametrize("name", sorted(sr.guard_cases()))
def test_each_guard_sets_exactly_its_flag(name):
    v, f, unit, want = sr.guard_cases()[name]
    acc, flags, n = sr.vertex_normals(v, f, unit)
    assert flags.tolist() == want
    assert ((n == 0).all(axis=1) == (flags != 0)).all() and np.isfinite(n).all()
    assert (acc[(flags & sr.RANGE) != 0] == 0).all() or name == "a NaN vertex"      # vertices 1, 2 also belong to a good face


def test_the_unit_from_the_bounding_box_keeps_every_face_below_the_guard():
    rs = np.random.RandomState(11)
    for scale in (1e-12, 1e-3, 1.0, 170.0, 1e6, 1e15):
        v = (rs.uniform(-1, 1, (40, 3)) * scale).astype(np.float32)
        lo, hi = v.min(axis=0), v.max(axis=0)
        v = np.concatenate([v, [lo, (hi[0], lo[1], lo[2]), (lo[0], hi[1], hi[2]), hi]]).astype(np.float32)     # the widest faces there can be
        f = np.concatenate([rs.randint(0, 40, (100, 3)), [(40, 41, 42), (41, 42, 43), (40, 43, 42)]]).astype(np.int32)
        unit = shade.normal_unit(v)
        assert math.frexp(unit)[0] == 0.5
        acc, flags, _ = sr.vertex_normals(v, f, unit)
        assert not (flags & sr.RANGE).any()
        assert np.abs(acc).max() > 2 ** 33                           # and the range is used: the widest face has at least 2^33 quanta
    assert shade.normal_unit(np.zeros((3, 3), np.float32)) == 1.0 and shade.normal_unit(np.full((2, 3), np.nan, np.float32)) == 1.0


# ---------------------------------------------------------------------------------------------- 2. the pixel arithmetic, analytically
LINEAR = shade.linear_tables(256)


def plane(side=4.0):
    h = side / 2
    v = np.asarray([(-h, -h, 0), (h, -h, 0), (h, h, 0), (-h, h, 0)], np.float32)
    return v, np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)


def check_plane_under_one_light(wrong=None):
    """A 4 x 4 plane facing the camera at z = 4, one light of intensity 8 at the camera's centre, K with a focal length of 16 and
    the principal point on the centre pixel of a 33 x 17 frame.  Centre pixel: p = (0, 0, 4), the face's cross product is
    (0, 0, +-16), so mm = 256, dd = 16, md = 64, root(mm * dd) = 64: every step is a power of two and E = 8 * 64 / (64 * 16) = 1/2
    = I / d^2 exactly.  Elsewhere p = (4 xn, 4 yn, 4) and the closed form is I * 4 / |p|^3; the kernel's route to it has 2 + 3
    roundings in xn, yn and p, 5 each in dd and md (md = 16 * 4 exactly here: 0), then mm * dd, the root (half weight), * dd,
    I * md, the quotient: below 16 roundings of 2^-53 each on a value of condition <= 3 in p -- 48 * 2^-53 relative."""
    H, W = 17, 33
    v, f = plane()
    K = centred_K(H, W, 16.0)
    for mode in (sr.SMOOTH, sr.FLAT):
        n = sr.vertex_normals(v, f, 1.0)[2]
        out = sr.render(v, f, grey(v), n, pose(t=(0, 0, 4))[None], K, H, W, ZNEAR, [(0, 0, 0, 8.0)], 0.0, *LINEAR, mode, wrong=wrong, with_E=True)
        E = out["E"][0]
        assert np.isfinite(E).sum() >= 200
        assert E[8, 16] == 0.5, E[8, 16]
        ys, xs = np.nonzero(np.isfinite(E))
        p = np.stack([(xs - 16) / 16.0 * 4, (ys - 8) / 16.0 * 4, np.full(len(xs), 4.0)], axis=1)
        want = 8.0 * 4.0 / np.linalg.norm(p, axis=1) ** 3
        assert np.abs(E[ys, xs] / want - 1).max() <= 48 * EPS
        assert out["unlit"].tolist() == [0]


def test_a_plane_under_one_light_follows_the_closed_form():
    check_plane_under_one_light()


def test_an_icosphere_lit_from_the_camera_follows_the_sphere():
    """Icosphere level 3, radius 1, centre (0, 0, 4), one light at the camera's centre, smooth normals.  At the drawn point p (on a
    facet) the sphere's law is E = I cos(theta) / |p|^2 with theta between the radial direction at p and the direction to the
    light.  The interpolated normal lies in the cone of the facet's three vertex normals and the radial direction in the cone of
    its three vertex directions, so the two differ by at most delta = the largest angle between a vertex normal and a vertex
    direction of one facet -- computed from the mesh.  |cos(theta +- delta) - cos(theta)| <= delta."""
    H, W = 48, 64
    v, f, _ = meshes.icosphere(3, 1.0)
    n = sr.vertex_normals(v, f, shade.normal_unit(v))[2]
    d = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1)[:, None]
    delta = max(np.arccos(np.clip(n[face] @ d[face].T, -1, 1)).max() for face in f)
    assert 0 < delta < 0.2
    K = centred_K(H, W, 60.0)
    I = 20.0
    out = sr.render(v, f, grey(v), n, pose(t=(0, 0, 4))[None], K, H, W, ZNEAR, [(0, 0, 0, I)], 0.0, *LINEAR, sr.SMOOTH, with_E=True)
    E, z = out["E"][0], out["depth"][0].astype(np.float64)
    ys, xs = np.nonzero(np.isfinite(E))
    assert len(ys) > 600
    p = np.stack([(xs - K[0, 2]) / 60.0 * z[ys, xs], (ys - K[1, 2]) / 60.0 * z[ys, xs], z[ys, xs]], axis=1)
    radial = p - (0, 0, 4)
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    dist = np.linalg.norm(p, axis=1)
    cos = np.maximum(0.0, -(radial * p).sum(axis=1) / dist)
    err = np.abs(E[ys, xs] - I * cos / dist ** 2)
    print(f"delta = {delta:.4f} rad, largest error {err.max() * dist.max() ** 2 / I:.4f} of the bound's unit")
    assert (err <= I * (delta + 1e-12) / dist ** 2).all()
    assert err.max() > 1e-6                                          # the facets do show: the bound is not idle


# ---------------------------------------------------------------------------------------------- 3. invariances
def box_scene():
    v, f, _ = meshes.three_boxes()
    rs = np.random.RandomState(5)
    P = np.stack([pose(rotation(rs), (0.1, -0.05, 5.0)), pose(rotation(rs), (-0.2, 0.1, 4.0))])
    return v, f, P, centred_K(48, 64, 70.0)


def check_winding_reversal(wrong=None):
    v, f, P, K = box_scene()
    lights = shade.blenderproc_lights(1.0)
    tables = shade.srgb_tables()
    g = f[:, [0, 2, 1]].copy()
    for mode in (sr.SMOOTH, sr.FLAT):
        a = sr.render(v, f, grey(v), sr.vertex_normals(v, f, 2.0 ** 20)[2], P, K, 48, 64, ZNEAR, lights, 0.0, *tables, mode, wrong=wrong)
        b = sr.render(v, g, grey(v), sr.vertex_normals(v, g, 2.0 ** 20)[2], P, K, 48, 64, ZNEAR, lights, 0.0, *tables, mode, wrong=wrong)
        assert (a["rgba"][..., 3] == 255).sum() > 400 and len(np.unique(a["rgba"][..., 0])) > 5
        assert a["rgba"].tobytes() == b["rgba"].tobytes() and a["depth"].tobytes() == b["depth"].tobytes()


def test_reversing_every_winding_changes_no_pixel():
    check_winding_reversal()


def test_a_light_behind_the_surface_adds_nothing():
    v, f = plane()
    K = centred_K(17, 33, 16.0)
    for mode in (sr.SMOOTH, sr.FLAT):
        n = sr.vertex_normals(v, f, 1.0)[2]
        args = (v, f, grey(v), n, pose(t=(0, 0, 4))[None], K, 17, 33, ZNEAR)
        behind = sr.render(*args, [(0.5, 0.2, 6.0, 1e6), (0, 0, 4.0, 1e6), (1.0, 1.0, 4.0, 1e6)], 0.25, *LINEAR, mode, with_E=True)
        E = behind["E"][0]
        assert (E[np.isfinite(E)] == 0.25).all() and np.isfinite(E).sum() > 200       # behind, at a surface point, in the surface's plane
        front = sr.render(*args, [(0.5, 0.2, 3.0, 1.0)], 0.25, *LINEAR, mode, with_E=True)["E"][0]
        assert (front[np.isfinite(front)] > 0.25).all()


def check_no_light_is_the_unshaded_resolve(wrong=None):
    v, f, c = meshes.icosphere(1, 1.0)
    rs = np.random.RandomState(9)
    P = np.stack([pose(rotation(rs), (0.0, 0.0, 2.0)), pose(rotation(rs), (0.3, 0.1, 6.0))])
    K = np.asarray([[70.0, 0.5, 30.0], [0, 66.0, 25.0], [0, 0, 1]], np.float32)
    base = raster_ref.render(v, f, c, P, K, 48, 64, ZNEAR)
    for mode in (sr.SMOOTH, sr.FLAT):
        got = sr.shade(base["vis"], base["xy"], base["vdepth"], f, c, v, np.zeros((len(v), 3)), P, K, np.zeros((0, 4)), 1.0, *LINEAR, mode, wrong=wrong)
        assert got[0].tobytes() == base["rgba"].tobytes() and got[1].tobytes() == base["depth"].tobytes()
    assert (base["rgba"][..., 3] == 255).sum() > 1000


def test_no_light_and_ambient_one_is_the_unshaded_resolve():
    check_no_light_is_the_unshaded_resolve()


def quarter_turn_pair(wrong=None, mode=sr.SMOOTH, with_lights=True):
    """three_boxes in front of a pinhole with square pixels and the principal point on the centre pixel of a 49 x 49 frame, drawn
    twice: as posed, and with the object AND the lights turned by 90 degrees about the optical axis -- (x, y, z) -> (-y, x, z),
    which maps the pixel grid onto itself: pixel (px, py) -> (48 - py, px)."""
    S = 49
    v, f, _ = meshes.three_boxes()
    K = centred_K(S, S, 100.0)
    Rz = np.asarray([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    P0 = pose(rotation(np.random.RandomState(2)), (0.0, 0.0, 5.0)).astype(np.float64)
    P1 = P0.copy()
    P1[:3] = Rz @ P0[:3]
    lights = np.asarray([(0.7, -0.4, 0.3, 30.0), (-1.0, 0.5, -0.5, 12.0)]) if with_lights else shade.blenderproc_lights(1.0)
    turned = lights.copy()
    turned[:, :3] = lights[:, :3] @ Rz.T
    n = sr.vertex_normals(v, f, 2.0 ** 20)[2]
    tables = shade.srgb_tables()
    a = sr.render(v, f, grey(v), n, P0[None].astype(np.float32), K, S, S, ZNEAR, lights, 0.0, *tables, mode, wrong=wrong, with_E=True)
    b = sr.render(v, f, grey(v), n, P1[None].astype(np.float32), K, S, S, ZNEAR, turned if with_lights else lights, 0.0, *tables, mode, wrong=wrong,
                  with_E=True)
    return a, b


def check_rigid_motion(wrong=None):
    """E at corresponding surface points is unchanged, within the rounding of the f32 depth in the key: p scales with z, E's
    condition in p is at most 3 + the cosine's, which the comparison keeps below 5 by leaving out grazing light -- 8 * 2^-24."""
    a, b = quarter_turn_pair(wrong)
    Ea, Eb = a["E"][0], np.rot90(b["E"][0], k=1)                    # b's pixel (48 - py, px) back onto (px, py)
    fa = np.where(np.isfinite(Ea), (a["vis"][0] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    fb = np.rot90(np.where(np.isfinite(b["E"][0]), (b["vis"][0] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1), k=1)
    both = (fa == fb) & (fa >= 0) & (Ea > 0.05 * Ea[np.isfinite(Ea)].max())
    assert both.sum() > 300, int(both.sum())
    assert np.abs(Eb[both] / Ea[both] - 1).max() <= 8 * 2.0 ** -24


def test_moving_object_and_lights_together_changes_no_irradiance():
    check_rigid_motion()


# ---------------------------------------------------------------------------------------------- 4. what it is for
def test_a_grey_box_stops_being_one_flat_value():
    """meshes.box painted one grey.  Unshaded: exactly one RGB value inside the mask.  Under the reference's lights (one unit =
    one metre) and sRGB tables, flat mode: the three visible faces have three different brightness levels -- their mean grey
    values lie more than ONE code value apart pairwise, the step below which an 8-bit image cannot tell two levels apart -- and
    each face is one smooth patch: no face spans as much as 40 code values, a sixth of the range."""
    v, f, _ = meshes.box((1.0, 0.6, 0.3))
    R = np.asarray([[0.8, -0.36, 0.48], [0.0, 0.8, 0.6], [-0.6, -0.48, 0.64]])
    assert np.allclose(R @ R.T, np.eye(3)) and np.linalg.det(R) > 0
    P, K = pose(R, (0, 0, 3.0))[None], centred_K(48, 64, 90.0)
    flat = raster_ref.render(v, f, grey(v), P, K, 48, 64, ZNEAR)
    inside = flat["rgba"][0, ..., 3] == 255
    assert inside.sum() > 400 and {tuple(p) for p in flat["rgba"][0][inside].tolist()} == {(102, 102, 102, 255)}
    lit = sr.render(v, f, grey(v), None, P, K, 48, 64, ZNEAR, shade.blenderproc_lights(1.0), 0.0, *shade.srgb_tables(), sr.FLAT)
    assert ((lit["rgba"][0, ..., 3] == 255) == inside).all() and lit["depth"].tobytes() == flat["depth"].tobytes() and lit["unlit"].tolist() == [0]
    quad = np.where(inside, (lit["vis"][0] & np.uint64(0xFFFFFFFF)).astype(np.int64) // 2, -1)
    seen = [k for k in range(6) if (quad == k).sum() > 30]
    assert len(seen) == 3
    values = [lit["rgba"][0][quad == k][:, 0].astype(np.float64) for k in seen]
    means = sorted(x.mean() for x in values)
    print("mean grey of the three faces:", means, "spans:", [x.max() - x.min() for x in values])
    assert min(means[1] - means[0], means[2] - means[1]) > 1 and 0 < means[0] and means[2] < 255
    assert max(x.max() - x.min() for x in values) < 40
    assert (lit["rgba"][0][inside][:, 0] == lit["rgba"][0][inside][:, 1]).all() and (lit["rgba"][0][inside][:, 0] == lit["rgba"][0][inside][:, 2]).all()


def test_two_views_a_quarter_turn_apart_differ():
    """three_boxes painted grey, the reference's lights, two views 90 degrees apart about the optical axis.  Unshaded, every
    pixel the two masks share is the same grey: the views differ in their outline alone.  Shaded (smooth and flat), more than
    HALF of the shared pixels differ -- the restatement gives 90 % and more (printed); a half leaves room for the light's
    symmetry under that very turn, which makes faces that swap roles look alike."""
    for mode in (sr.SMOOTH, sr.FLAT):
        a, b = quarter_turn_pair(mode=mode, with_lights=False)
        ma, mb = a["rgba"][0, ..., 3] == 255, b["rgba"][0, ..., 3] == 255
        common = ma & mb
        assert common.sum() > 150 and (ma ^ mb).sum() > 50
        share = (a["rgba"][0][common] != b["rgba"][0][common]).any(axis=1).mean()
        print(f"mode {mode}: {share:.3f} of {int(common.sum())} shared pixels differ")
        assert share > 0.5


# ---------------------------------------------------------------------------------------------- 5. tables, lights, files
def check_srgb_round_trip(wrong=None):
    """decode then encode at irradiance 1 gives every colour byte back: at T = 4096 one level is 0.80 code values at the curve's
    steepest, so the nearest level is within 0.40 < 1/2 of the byte's own value (srgb_tables' docstring)."""
    decode, encode = shade.srgb_tables(4096)
    assert decode[0] == 0 and decode[255] == 1 and (np.diff(decode) > 0).all() and encode[0] == 0 and encode[-1] == 255
    assert (np.diff(encode.astype(int)) >= 0).all() and np.diff(encode.astype(int)).max() <= 1
    assert 12.92 * 255 / 4095 < 1
    v, f = plane()
    col = np.asarray([(0, 1, 2), (0, 1, 2), (255, 254, 253), (255, 254, 253)], np.uint8)    # a ramp through every byte region
    K = centred_K(17, 33, 16.0)
    base = raster_ref.render(v, f, col, pose(t=(0, 0, 4))[None], K, 17, 33, ZNEAR)
    got = sr.shade(base["vis"], base["xy"], base["vdepth"], f, col, v, None, pose(t=(0, 0, 4))[None], K, [], 1.0, decode, encode, sr.FLAT, wrong=wrong)
    assert len(np.unique(base["rgba"][..., 0])) > 14 and got[0].tobytes() == base["rgba"].tobytes()
    x = np.rint(decode * 4095).astype(int) if wrong is None else np.floor(decode * 4095).astype(int)
    assert (encode[x] == np.arange(256)).all()


def test_srgb_tables_round_trip():
    check_srgb_round_trip()
    d, e = shade.linear_tables(256)
    assert (e == np.arange(256)).all() and (np.floor(d * 255 + 0.5) == np.arange(256)).all()
    for T in (255, 65537):
        with pytest.raises(ValueError):
            shade.srgb_tables(T)
        with pytest.raises(ValueError):
            shade.linear_tables(T)
    assert len(shade.srgb_tables(65536)[1]) == 65536


def test_blenderproc_lights():
    """x, y in {-1, 1} and z in {0, 1} metres in Blender's frame, in the reference's loop order; OpenCV's frame flips y and z."""
    L = shade.blenderproc_lights(1000.0)
    blender = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (0, 1)]
    assert L.shape == (8, 4) and L.dtype == np.float64
    assert L[:, :3].tolist() == [[1000.0 * x, -1000.0 * y, -1000.0 * z] for x, y, z in blender]
    assert (L[:, 2] <= 0).all() and (L[:, 3] == 50.0 / (4.0 * math.pi ** 2) * 1000.0 * 1000.0).all()
    assert shade.blenderproc_lights(1.0, watts=4 * math.pi ** 2)[:, 3].tolist() == [1.0] * 8


PLY_HEAD = "ply\nformat {fmt} 1.0\ncomment made for a test\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n{normals}" \
           "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "no normals"])
def test_load_ply_with_normals(tmp_path, fmt, with_normals):
    v, f = plane()
    n = np.asarray([(0, 0, -1), (0.6, 0, -0.8), (0, 0.28, -0.96), (0, 0, 1)], np.float32)
    c = np.asarray([(1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)], np.uint8)
    head = PLY_HEAD.format(fmt=fmt, normals="property float nx\nproperty float ny\nproperty float nz\n" if with_normals else "").encode()
    if fmt == "ascii":
        rows = [" ".join(map(str, list(v[i]) + (list(n[i]) if with_normals else []) + list(c[i]))) for i in range(4)]
        body = ("\n".join(rows + ["3 " + " ".join(map(str, t)) for t in f]) + "\n").encode()
    else:
        body = b"".join(v[i].tobytes() + (n[i].tobytes() if with_normals else b"") + c[i].tobytes() for i in range(4))
        body += b"".join(b"\x03" + t.astype("<i4").tobytes() for t in f)
    path = tmp_path / "model.ply"
    path.write_bytes(head + body)
    gv, gf, gc, gn = shade.load_ply_with_normals(path)
    assert (gv == v).all() and (gf == f).all() and (gc == c).all()
    if with_normals:
        assert gn.dtype == np.float64 and gn.shape == (4, 3) and (gn == n.astype(np.float64)).all()
    else:
        assert gn is None
        with pytest.raises(ValueError, match="carries no normals"):
            shade.ShadedMeshTemplates([(str(path), np.eye(4)[None])], normals="file")
    t = shade.ShadedMeshTemplates([(str(path), np.eye(4)[None])], normals="file" if with_normals else "smooth")
    assert len(t) == 1 and t.renderer.lights.shape == (8, 4) and t.colour == (102, 102, 102)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        shade.ShadedMeshTemplates([(str(path), np.eye(4)[None])], device="cpu").render(0)


def test_cpu_input_has_no_fallback_and_wrong_arguments_are_rejected():
    import torch

    v, f = plane()
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        shade.vertex_normals(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        shade.ShadedMeshRenderer()(torch.from_numpy(v), torch.from_numpy(f), None, torch.eye(4)[None], colour=(1, 2, 3))
    with pytest.raises(ValueError, match="at most 16 lights"):
        shade.ShadedMeshRenderer(lights=np.zeros((17, 4)))
    with pytest.raises(ValueError, match="mode"):
        shade.ShadedMeshRenderer(mode="phong")
    with pytest.raises(ValueError, match="tables"):
        shade.ShadedMeshRenderer(tables=(np.zeros(255), np.zeros(256, np.uint8)))
    with pytest.raises(ValueError, match="normals must be"):
        shade.ShadedMeshTemplates([], normals="vertex")


# ---------------------------------------------------------------------------------------------- 6. wrong shaders
REJECTED_BY = {"no_flip": check_winding_reversal,                    # the reversed mesh turns its back on every light
               "unnormalised": check_cube_and_octahedron,            # the normals are the raw sums
               "falloff_1_over_d": check_plane_under_one_light,      # the centre pixel gets I / d = 2
               "object_lights": check_plane_under_one_light,         # the light at the camera's centre lands in the plane
               "screen_weights": check_no_light_is_the_unshaded_resolve,   # the colour bytes themselves move
               "wrong_key_half": check_no_light_is_the_unshaded_resolve,   # depth bits are no face index
               "truncate_encode": check_srgb_round_trip}             # a byte falls one short


def test_every_wrong_shader_has_a_check():
    assert sorted(REJECTED_BY) == sorted(sr.WRONG) and len(sr.WRONG) >= 7
    with pytest.raises(ValueError):
        sr.vertex_normals(*plane(), 1.0, wrong="phong")


@pytest.mark.parametrize("name", sr.WRONG)
def test_the_checks_reject_wrong_shaders(name):
    with pytest.raises(AssertionError):
        REJECTED_BY[name](wrong=name)


def test_object_lights_are_also_rejected_by_the_rigid_motion():
    with pytest.raises(AssertionError):
        check_rigid_motion(wrong="object_lights")
