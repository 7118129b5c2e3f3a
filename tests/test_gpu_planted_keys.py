"""GPU: one hand-edited key buffer through the three resolves -- gpr_resolve, gpt_resolve and gpl_shade in both modes.

What the three kernels do with a pixel's key before they colour it is one function (gp_raster_geom.h: resolve_pixel): which keys
are background, the triangle set-up with its vertex swap, the weights, the depth word.  This test plants a key for every way out
of that function and for both values of the swap, at the smallest size that reaches them all, and holds each kernel to its numpy
restatement bit for bit and the three to each other."""
import numpy as np
import pytest

from gigapose_testing import meshes, raster_ref
from gigapose_testing import shade_ref as sr
from gigapose_testing import texture_ref as tr
from gigapose_testing.gpu_cases import ZNEAR, assert_bits, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu
DEPTH = np.float32(2.5)                                              # the depth word of every planted key


def swapped(xy_n, faces, f):
    tri, _ = raster_ref.setup(xy_n, faces, f, len(xy_n))
    return None if tri is None else tri[0][1] != int(faces[f][1])


@pytest.mark.parametrize("frame", [(48, 64), (47, 63)], ids=["64x48: 12 workgroups", "63x47: a partial last one"])
def test_planted_keys_through_the_three_resolves(frame):
    """Mesh: icosphere(1) with the corner order of every second face reversed (the faces drawn show both values of Tri::swapped),
    + a face of zero area + a face that names vertex V.  Two views; in view 1 one vertex lies behind znear (its xy is the bad
    coordinate, as gpr_project writes it).  Planted over the keys gpr_raster drew, in both views: a face word of F and one of
    0xffffffff, the zero-area face, the out-of-range face, a valid face at a pixel outside its triangle, a key each at the first
    and the last pixel of the frame, and a face that uses the vertex which view 1 lost (drawn in view 0, background in view 1)."""
    from gigapose_amd import render, shade, texture

    H, W = frame
    v, f, c = meshes.icosphere(1, 0.6)
    V = len(v)
    f = f.copy()
    f[1::2] = f[1::2][:, [0, 2, 1]]
    f = np.concatenate([f, [(0, 0, 1), (0, 1, V)]]).astype(np.int32)
    F = len(f)
    zero_area, out_of_range = F - 2, F - 1
    rs = np.random.RandomState(5)
    P = np.stack([pose(rotation(rs), (0.03, -0.02, 2.2)), pose(rotation(rs), (-0.05, 0.04, 2.6))]).astype(np.float32)
    K = np.asarray([[60.0, 0.25, (W - 1) / 2], [0, 61.0, (H - 1) / 2], [0, 0, 1]], np.float32)
    xy, z = raster_ref.project(v, P, K, ZNEAR)
    # the vertex view 1 loses: the first corner of the face at view 0's centre, which view 1 draws as well
    first = render.raster(_t(xy), _t(z), _t(f), H, W)[0].cpu().numpy().view(np.uint64)
    assert (first[:, H // 2, W // 2] != raster_ref.EMPTY_KEY).all()
    lost_face = int(first[0, H // 2, W // 2] & np.uint64(0xFFFFFFFF))
    lost = int(f[lost_face][0])
    xy[1, lost], z[1, lost] = raster_ref.BAD_COORD, np.float32(-0.5)
    vis, clipped = render.raster(_t(xy), _t(z), _t(f), H, W)
    uses_lost = (f == lost).any(axis=1)
    assert clipped.tolist() == [1, 1 + int(uses_lost[:F - 1].sum())] and uses_lost.sum() >= 5
    keys = vis.cpu().numpy().view(np.uint64).copy()
    owner = np.where(keys != raster_ref.EMPTY_KEY, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    drawn_faces = [np.unique(owner[n][owner[n] >= 0]) for n in range(2)]
    for n in range(2):                                               # both windings are on screen before anything is planted
        assert {swapped(xy[n], f, int(k)) for k in drawn_faces[n]} == {False, True} and (owner[n] >= 0).sum() > 300
    assert not np.isin(np.nonzero(uses_lost)[0], drawn_faces[1]).any()
    cy, cx = H // 2, W // 2
    assert (owner[0, cy:cy + 2, cx:cx + 4] >= 0).all() and (owner[:, :2] == -1).all() and (owner[:, H - 1] == -1).all()
    bits = np.uint64(DEPTH.view(np.uint32)) << np.uint64(32)
    intact = drawn_faces[0][~uses_lost[drawn_faces[0]]]               # faces both views can set up
    even, odd = int(intact[intact % 2 == 0][0]), int(intact[intact % 2 == 1][0])
    background = {(cy, cx): F, (cy, cx + 1): 0xFFFFFFFF, (cy, cx + 2): zero_area, (cy, cx + 3): out_of_range}
    covered = {(1, 5): int(intact[-1]), (0, 0): even, (H - 1, W - 1): odd, (cy + 1, cx): lost_face}
    for (y, x), face in list(background.items()) + list(covered.items()):
        keys[:, y, x] = bits | np.uint64(face)
    planted = _t(keys)

    uv = rs.uniform(0.0, 1.0, (F, 3, 2)).astype(np.float32)
    tex = tr.noise_texture(8, 8, seed=3)
    pyramid = texture.build_mips(_t(tex))
    normals = sr.vertex_normals(v, f, shade.normal_unit(v))[2]
    lights = np.asarray([(0.5, -0.4, -1.0, 3.0), (-1.0, 0.8, 0.5, 2.0)])
    srgb, linear = shade.srgb_tables(4096), shade.linear_tables(256)
    dxy, dz, df = _t(xy), _t(z), _t(f)

    def shaded(mode, rows, ambient, tables):
        got = shade.shade(planted, dxy, dz, df, _t(c), _t(v), _t(normals), _t(P), K, rows, ambient, _t(tables[0]), _t(tables[1]), mode)
        want = sr.shade(keys, xy, z, f, c, v, normals, P, K, rows if rows is not None else [], ambient, tables[0], tables[1], mode)
        for g, w, name in zip(got, want, ("rgba", "depth", "unlit")):
            assert_bits(g, w, f"gpl_shade, mode {mode}, {0 if rows is None else len(rows)} lights: {name}")
        return got[0].cpu().numpy(), got[1].cpu().numpy()

    out = {"gpr_resolve": tuple(t.cpu().numpy() for t in render.resolve(planted, dxy, dz, df, _t(c))),
           "gpt_resolve": tuple(t.cpu().numpy() for t in texture.resolve_textured(planted, dxy, dz, df, _t(uv), pyramid, tex.shape[:2]))}
    for name, want in (("gpr_resolve", raster_ref.resolve(keys, xy, z, f, c)),
                       ("gpt_resolve", tr.resolve(keys, xy, z, f, uv, tr.build_mips(tex), *tex.shape[:2]))):
        assert_bits(out[name][0], want[0], f"{name}: rgba")
        assert_bits(out[name][1], want[1], f"{name}: depth")
    for mode, label in ((sr.SMOOTH, "smooth"), (sr.FLAT, "flat")):
        out[f"gpl_shade, {label}"] = shaded(mode, lights, 0.1, srgb)
        plain = shaded(mode, None, 1.0, linear)
        assert_bits(plain[0], out["gpr_resolve"][0], f"gpl_shade, {label}, no light, ambient 1, linear tables against gpr_resolve: rgba")
        assert_bits(plain[1], out["gpr_resolve"][1], f"gpl_shade, {label}, no light, ambient 1, linear tables against gpr_resolve: depth")

    rgba, depth = out["gpr_resolve"]
    for name, (other, other_depth) in out.items():                   # one gate, one depth word
        assert_bits(other[..., 3], rgba[..., 3], f"{name} against gpr_resolve: alpha")
        assert_bits(other_depth, depth, f"{name} against gpr_resolve: depth")
        assert (other[rgba[..., 3] == 0] == 0).all()
    for y, x in background:
        assert (rgba[:, y, x] == 0).all() and (depth[:, y, x] == 0).all()
    for (y, x), face in covered.items():
        views = [0] if face == lost_face else [0, 1]
        assert (rgba[views, y, x, 3] == 255).all() and (depth[views, y, x] == DEPTH).all()
    assert rgba[1, cy + 1, cx].tolist() == [0, 0, 0, 0] and depth[1, cy + 1, cx] == 0
    assert set(np.unique(rgba[..., 3])) == {0, 255} and ((rgba[..., 3] == 255) == (depth > 0)).all()
