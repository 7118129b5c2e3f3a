"""GPU: textured mesh + poses -> RGBA renders and depth (libgigapose_texture.so, gigapose_amd/texture.py).

The two kernels against the numpy restatement (gigapose_testing/texture_ref.py, written from the header) bit for bit; level
selection and the UV conventions seen from outside (a hand-written pyramid, a texture reproduced texel for pixel); invariances;
bad UVs; a constant texture against the coloured renderer; a key buffer past 2^31 bytes; chunking; and TexturedMeshTemplates ->
set_template_data -> predict against RenderedTemplates on the saved PNGs."""
import numpy as np
import pytest
import torch

from gigapose_testing import factory, meshes, raster_ref
from gigapose_testing import synthetic as syn
from gigapose_testing import texture_ref as tr
from gigapose_testing.gpu_cases import DEV, K_SMALL, ZNEAR, assert_bits, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu


def frontal_K(H, W, focal=256.0, cx=None, cy=None):
    return np.asarray([[focal, 0, (W - 1) / 2 if cx is None else cx], [0, focal, (H - 1) / 2 if cy is None else cy], [0, 0, 1]], np.float32)


def at_depth(d):
    return pose(np.eye(3), (0.0, 0.0, d))[None].astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. gpt_build_mips
@pytest.mark.parametrize("size", [(1, 1), (1, 256), (256, 1), (5, 7), (64, 64), (129, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_build_mips_equals_the_restatement(size):
    from gigapose_amd import _lib, texture

    rgb = tr.noise_texture(*size, seed=size[0] + size[1])
    want = tr.build_mips(rgb)
    assert len(want) == texture.mip_texels(*size)
    got = texture.build_mips(_t(rgb))
    assert got.dtype == torch.int32 and got.is_cuda
    assert_bits(got.cpu().numpy().view(np.uint32), want, "pyramid")
    dirty = torch.full((len(want),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)                      # every word is written
    texture._call("gpt_build_mips", _lib.ptr(_t(rgb)), _lib.i(size[0]), _lib.i(size[1]), _lib.ptr(dirty), _lib.stream_ptr())
    assert_bits(dirty.cpu().numpy().view(np.uint32), want, "pyramid over garbage")


# ---------------------------------------------------------------------------------------------- 2. gpt_resolve
def factor(pixels, H, W):
    for h in range(2, H - 4):
        if pixels % h == 0 and pixels // h <= W - 4:
            return pixels // h, h
    return None


def screen_scenes(H, W):
    """name -> (xy (V,2) int32, depth (V,) f32, faces (F,3) int32, corner_uv (F,3,2) f32): hand-made screen coordinates, one view
    each.  The fans of tests/test_gpu_render.py (both windings, shared edges), triangles at threshold - 1, threshold and
    threshold + 1 pixels of gpr_small_triangle_pixels() and one far larger, and a plane seen almost edge-on."""
    from gigapose_amd import render

    rs = np.random.RandomState(H * 5 + W)
    T = render.small_triangle_pixels()
    out = {}
    for k in range(6):
        p, c = meshes.screen_polygon(rs, H, W, on_centres=k % 2 == 0)
        for about_centre in (False, True):
            xy = np.concatenate([p, c]).astype(np.int32)
            faces = meshes.fan_faces(len(p), about_centre)
            if k % 3 == 2:
                faces = faces[:, ::-1].copy()                        # the other winding
            spread = (0.2, 1.5, 6.0)[k % 3]                          # UVs inside [0, 1], a little outside, several repeats
            uv = rs.uniform(0.5 - spread, 0.5 + spread, (len(faces), 3, 2)).astype(np.float32)
            out[f"polygon {k}, fan about {'the centre' if about_centre else 'vertex 0'}"] = (xy, rs.uniform(1, 3, len(xy)).astype(np.float32), faces, uv)
    pts, faces, z = [], [], []
    for i, pixels in enumerate((T - 1, T, T + 1)):
        w, h = factor(pixels, H, W)
        faces.append([len(pts) + j for j in range(3)])
        pts += [((1 + i) * 256, (2 + i) * 256), ((1 + i + w - 1) * 256, (2 + i) * 256), ((1 + i) * 256, (2 + i + h - 1) * 256)]
        z += [0.9 + 0.3 * i, 2.5, 1.4]
    faces.append([len(pts) + j for j in range(3)])
    pts += [(-5 * W * 256 + 37, -4 * H * 256 + 11), (6 * W * 256 + 5, -5 * H * 256), (W * 128 + 77, H * 230 + 3)]    # ten times the frame
    z += [9.0, 7.0, 8.0]
    xy, faces = np.asarray(pts, np.int32), np.asarray(faces, np.int32)
    assert [raster_ref.box_pixels(xy, faces, i, H, W) for i in range(3)] == [T - 1, T, T + 1]
    out["triangles across the threshold"] = (xy, np.asarray(z, np.float32), faces, rs.uniform(-0.3, 1.3, (4, 3, 2)).astype(np.float32))
    # a plane whose horizon lies just beyond its far edge: 1 / depth falls from 100 to 0.001 across the triangle, and reaches 0
    # within a pixel of the edge 1 -> 2, so the right neighbour of the pixels along that edge has q <= 0
    xy = np.asarray([(5 * 256, 5 * 256 + 9), ((W - 5) * 256 + 31, 8 * 256), ((W - 7) * 256, (H - 4) * 256 + 100)], np.int32)
    out["horizon"] = (xy, np.asarray([0.01, 1000.0, 1000.0], np.float32), np.asarray([(0, 1, 2)], np.int32),
                      np.asarray([[(0.0, 0.0), (3.0, 0.2), (2.5, 4.0)]], np.float32))
    return out


def mesh_views(H, W):
    """name -> (vertices, faces, corner_uv, poses, K): the UV box and the UV icosphere near, far and at a slant."""
    K = frontal_K(H, W, focal=0.9 * W)
    rs = np.random.RandomState(12)
    box_poses = np.stack([pose(rotation(rs), (0.05, -0.03, d)) for d in (1.3, 4.0, 30.0)]).astype(np.float32)
    ball_poses = np.stack([pose(rotation(rs), (-0.1, 0.08, d)) for d in (1.6, 6.0, 70.0)]).astype(np.float32)
    return {"UV box": meshes.uv_box((1.0, 0.6, 0.3)) + (box_poses, K), "UV icosphere": meshes.uv_icosphere(1, 0.7) + (ball_poses, K)}


TEXTURE_SIZES = [(8, 8), (5, 7), (64, 64), (1, 1)]


@pytest.fixture(scope="module", params=[(48, 64), (120, 160)], ids=["64x48", "160x120"])
def resolved(request):
    """Every scene resolved with every texture size, once by the kernel and once by the restatement, from the SAME keys (the
    kernel's own raster; tests/test_gpu_render.py holds those to raster_ref)."""
    from gigapose_amd import render, texture

    H, W = request.param
    cases = []
    for name, (xy, z, faces, uv) in screen_scenes(H, W).items():
        cases.append((name, xy[None], z[None], faces, uv))
    for name, (v, f, uv, poses, K) in mesh_views(H, W).items():
        xy, z = raster_ref.project(v, poses, K, ZNEAR)
        cases.append((name, xy, z, f, uv))
    res = {}
    for name, xy, z, faces, uv in cases:
        d_xy, d_z, d_f, d_uv = _t(xy), _t(z), _t(faces), _t(uv)
        vis, _ = render.raster(d_xy, d_z, d_f, H, W)
        keys = vis.cpu().numpy().view(np.uint64)
        for Ht, Wt in TEXTURE_SIZES:
            if (Ht, Wt) != (64, 64) and not name.startswith("UV") and not name.startswith("horizon"):
                continue                                             # the fans are drawn with one texture
            rgb = tr.noise_texture(Ht, Wt, seed=Ht * 31 + Wt)
            pyramid = texture.build_mips(_t(rgb))
            rgba, depth = texture.resolve_textured(vis, d_xy, d_z, d_f, d_uv, pyramid, (Ht, Wt))
            want = tr.resolve(keys, xy, z, faces, uv, pyramid.cpu().numpy(), Ht, Wt)
            res[f"{name}, texture {Ht} x {Wt}"] = dict(got=(rgba.cpu().numpy(), depth.cpu().numpy()), want=want,
                                                       info=tr.inspect(keys, xy, z, faces, uv, Ht, Wt), top=tr.mip_levels(Ht, Wt) - 1)
    return dict(H=H, W=W, res=res)


def test_resolve_equals_the_restatement(resolved):
    for name, r in resolved["res"].items():
        assert_bits(r["got"][0], r["want"][0], f"rgba of '{name}'")
        assert_bits(r["got"][1], r["want"][1], f"depth of '{name}'")
        a = r["got"][0][..., 3]
        assert set(np.unique(a)) == {0, 255}, name
        assert (r["got"][1][a == 0] == 0).all() and (r["got"][1][a == 255] > 0).all() and (r["got"][0][a == 0] == 0).all()
        assert ((a == 255) == r["info"]["covered"]).all()


def test_the_scenes_exercise_every_branch(resolved):
    """Magnification, a blend of two levels (of levels 0 and 1, and of higher ones), the top level alone, the q <= 0 neighbour
    rule and UVs outside [0, 1] all occur among the pixels compared above."""
    seen = dict(magnified=0, blended=0, blended_above_0=0, top_alone=0, no_rho=0, wrapped=0)
    for name, r in resolved["res"].items():
        i, top = r["info"], r["top"]
        c = i["covered"] & ~i["bad"]
        assert not i["bad"].any(), name
        seen["magnified"] += int((c & (i["rho2"] < 1.0)).sum())
        seen["blended"] += int((c & i["two"]).sum())
        seen["blended_above_0"] += int((c & i["two"] & (i["l0"] >= 1)).sum())
        seen["top_alone"] += int((c & ~i["two"] & (i["l0"] == top) & (i["rho2"] >= 1.0)).sum()) if top > 0 else 0
        seen["no_rho"] += int((c & np.isnan(i["rho2"])).sum()) if name.startswith("horizon") else 0
        with np.errstate(invalid="ignore"):
            seen["wrapped"] += int((c & ((i["u"] < 0) | (i["u"] > 1) | (i["v"] < 0) | (i["v"] > 1))).sum())
    print(seen)
    assert all(seen[k] > 20 for k in ("magnified", "blended", "blended_above_0", "top_alone", "wrapped")), seen
    assert seen["no_rho"] >= 3, seen


# ---------------------------------------------------------------------------------------------- 3. level selection from outside
def draw_quad(tex_or_pyramid, quad, K, H, W, d, uv_min=(0.0, 0.0), uv_max=(1.0, 1.0)):
    from gigapose_amd import texture

    v, f, uv = meshes.uv_quad(quad, uv_min=uv_min, uv_max=uv_max)
    out = texture.TexturedMeshRenderer(H, W, K, ZNEAR)(_t(v), _t(f), _t(uv), tex_or_pyramid, _t(at_depth(d)))
    assert out["clipped"].tolist() == [0]
    xy, z = raster_ref.project(v, at_depth(d), K, ZNEAR)
    vis, _ = raster_ref.raster(xy, z, f, H, W)
    return out, (vis, xy, z, f, uv)


def test_level_selection_seen_from_outside():
    """A pyramid written by hand: level l of a 64 x 64 texture is the constant colour (20 l, 0, 255 - 20 l).  A unit quad seen
    head-on with a 256 px focal length at depth d shows d / 4 texels per pixel: 1, 2 and 4 return the colours of levels 0, 1 and
    2 (rho2 sits on a power of four to a rounding error, so either that level alone or its blend with a weight within 1e-9 of 0
    or 1: the same byte), 3 returns the blend w = (9 / 4 - 1) / 3 of levels 1 and 2."""
    H, W = 120, 160
    sizes = tr.mip_sizes(64, 64)
    colours = [(20 * l, 0, 255 - 20 * l) for l in range(len(sizes))]
    pyramid = tr.pack_levels([tr.constant_texture(h, w, c) for (h, w), c in zip(sizes, colours)])
    d_pyr = _t(pyramid.view(np.int32))
    w = (9.0 / 4.0 - 1.0) / 3.0
    blend = tuple(int(np.floor((1 - w) * a + w * b + 0.5)) for a, b in zip(colours[1], colours[2]))
    assert blend == (28, 0, 227)
    for d, want in ((4.0, colours[0]), (8.0, colours[1]), (16.0, colours[2]), (12.0, blend)):
        out, (vis, xy, z, f, uv) = draw_quad((d_pyr, (64, 64)), (1.0, 1.0), frontal_K(H, W), H, W, d)
        ref_rgba, ref_depth = tr.resolve(vis, xy, z, f, uv, pyramid, 64, 64)
        assert_bits(out["rgba"], ref_rgba, f"rgba at depth {d}")
        assert_bits(out["depth"], ref_depth, f"depth at depth {d}")
        rgba = out["rgba"][0].cpu().numpy()
        a = rgba[..., 3] == 255
        side = {4.0: 64, 8.0: 32, 16.0: 16, 12.0: 22}[d]               # 256 / d pixels about the principal point at 79.5, 59.5
        assert a.sum() == side * side, (d, int(a.sum()))
        got = set(map(tuple, rgba[a][:, :3].tolist()))
        assert got == {want}, f"{d / 4} texels per pixel: {got} vs {want}"


# ---------------------------------------------------------------------------------------------- 4. identity
def test_a_texture_is_reproduced_texel_for_pixel():
    """A 32 x 24 noise texture on a quad of 32 x 24 pixels whose texel centres fall on pixel centres: the frame shows the
    texture, upright (UV origin bottom-left, image row 0 on top).  At half the size it shows level 1 of the pyramid."""
    H, W = 48, 64
    tex = tr.noise_texture(24, 32, seed=8)
    level1 = tr.split_levels(tr.build_mips(tex), 24, 32)[1][..., :3]
    x0, y0 = 20, 10
    out, _ = draw_quad(_t(tex), (1.0, 0.75), frontal_K(H, W, cx=x0 + 15.5, cy=y0 + 11.5), H, W, 8.0)
    rgba = out["rgba"][0].cpu().numpy()
    assert (rgba[y0:y0 + 24, x0:x0 + 32, 3] == 255).all() and int((rgba[..., 3] == 255).sum()) == 24 * 32
    np.testing.assert_array_equal(rgba[y0:y0 + 24, x0:x0 + 32, :3], tex)
    out, _ = draw_quad(_t(tex), (1.0, 0.75), frontal_K(H, W, cx=x0 + 7.5, cy=y0 + 5.5), H, W, 16.0)
    rgba = out["rgba"][0].cpu().numpy()
    assert int((rgba[..., 3] == 255).sum()) == 12 * 16
    np.testing.assert_array_equal(rgba[y0:y0 + 12, x0:x0 + 16, :3], level1)


# ---------------------------------------------------------------------------------------------- 5. invariances
@pytest.fixture(scope="module")
def box_views():
    from gigapose_amd import texture

    v, f, uv = meshes.uv_box((1.0, 0.6, 0.3))
    rs = np.random.RandomState(404)
    poses = np.stack([pose(rotation(rs), (rs.uniform(-.2, .2), rs.uniform(-.1, .1), rs.uniform(1.5, 6))) for _ in range(5)]).astype(np.float32)
    tex = tr.noise_texture(64, 48, seed=3)
    r = texture.TexturedMeshRenderer(240, 320, K_SMALL, ZNEAR)
    return dict(v=v, f=f, uv=uv, poses=poses, tex=tex, r=r, out=r(_t(v), _t(f), _t(uv), _t(tex), _t(poses)))


def test_box_views_equal_the_restatement(box_views):
    s = box_views
    want = tr.render(s["v"], s["f"], s["uv"], s["tex"], s["poses"][:2], K_SMALL, 240, 320, ZNEAR)
    assert_bits(s["out"]["rgba"][:2], want["rgba"], "rgba")
    assert_bits(s["out"]["depth"][:2], want["depth"], "depth")
    assert s["out"]["clipped"].tolist() == [0] * 5 and (want["rgba"][..., 3] == 255).sum() > 2000


def test_invariances(box_views):
    s = box_views
    v, f, uv, r = s["v"], s["f"], s["uv"], s["r"]
    tex, poses = _t(s["tex"]), _t(s["poses"])
    rev = r(_t(v), _t(f[::-1].copy()), _t(uv[::-1].copy()), tex, poses)
    flip = r(_t(v), _t(f[:, [0, 2, 1]].copy()), _t(uv[:, [0, 2, 1]].copy()), tex, poses)
    v24, f24, uv24 = meshes.uv_box((1.0, 0.6, 0.3), shared=False)
    vertex_uv = np.zeros((24, 2), np.float32)
    vertex_uv[f24.reshape(-1)] = uv24.reshape(-1, 2)
    from gigapose_amd import texture

    gathered = texture.corner_uv_from_vertices(vertex_uv, f24)
    np.testing.assert_array_equal(gathered, uv)                      # 24 vertices carry one UV each; the 8 shared ones could not
    dup = r(_t(v24), _t(f24), _t(gathered), tex, poses)
    for key in ("rgba", "depth", "clipped"):
        assert_bits(rev[key], s["out"][key], f"{key}, reversed face order")
        assert_bits(flip[key], s["out"][key], f"{key}, flipped winding")
        assert_bits(dup[key], s["out"][key], f"{key}, duplicated seam vertices")


def test_chunking_and_determinism(box_views):
    s = box_views
    args = (_t(s["v"]), _t(s["f"]), _t(s["uv"]), _t(s["tex"]), _t(s["poses"]))
    again = s["r"](*args)
    chunked = s["r"](*args, views_per_call=2)
    from gigapose_amd import texture

    prebuilt = s["r"](*args[:3], (texture.build_mips(args[3]), s["tex"].shape[:2]), args[4])
    for key in ("rgba", "depth", "clipped"):
        assert_bits(again[key], s["out"][key], f"{key}, second call")
        assert_bits(chunked[key], s["out"][key], f"{key}, two views per call")
        assert_bits(prebuilt[key], s["out"][key], f"{key}, pyramid built before")


# ---------------------------------------------------------------------------------------------- 6. bad UVs
def test_bad_uvs_blacken_exactly_their_faces():
    """NaN, +-inf, 1e30 and GPT_MAX_UV + 1 ulp in ONE corner each of five faces of an icosphere: exactly the pixels those faces
    own are 0, 0, 0 with alpha 255 and their depth; GPT_MAX_UV - 1 ulp and GPT_MAX_UV itself are ordinary (if large)
    coordinates; the image equals the restatement."""
    from gigapose_amd import render, texture

    H, W = 120, 160
    v, f, uv = meshes.uv_icosphere(1, 1.0)
    K = frontal_K(H, W, focal=140.0)
    P = pose(rotation(np.random.RandomState(5)), (0.0, 0.0, 3.0))[None].astype(np.float32)
    xy, z = raster_ref.project(v, P, K, ZNEAR)
    vis, _ = raster_ref.raster(xy, z, f, H, W)
    owner = np.where(vis[0] != raster_ref.EMPTY_KEY, (vis[0] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    faces_seen, counts = np.unique(owner[owner >= 0], return_counts=True)
    big = faces_seen[np.argsort(-counts)][:7]
    assert counts.min() >= 1 and len(big) == 7 and np.sort(-counts)[6] <= -30
    top_uv = np.float32(texture.MAX_UV)
    values = [np.nan, np.inf, -np.inf, 1e30, np.nextafter(top_uv, np.float32(np.inf)), np.nextafter(top_uv, np.float32(0)), -top_uv]
    uv = uv.copy()
    for k, (face, val) in enumerate(zip(big, values)):
        uv[face, k % 3, k % 2] = val
    tex = np.maximum(tr.noise_texture(8, 8, seed=1), 16)             # no black texel
    d_xy, d_z, d_f = _t(xy), _t(z), _t(f)
    keys, _ = render.raster(d_xy, d_z, d_f, H, W)
    assert_bits(keys.cpu().numpy().view(np.uint64), vis, "keys")
    pyramid = texture.build_mips(_t(tex))
    rgba, depth = texture.resolve_textured(keys, d_xy, d_z, d_f, _t(uv), pyramid, (8, 8))
    torch.cuda.synchronize()                                        # the launch completes
    want_rgba, want_depth = tr.resolve(vis, xy, z, f, uv, pyramid.cpu().numpy(), 8, 8)
    assert_bits(rgba, want_rgba, "rgba")
    assert_bits(depth, want_depth, "depth")
    rgba, depth = rgba[0].cpu().numpy(), depth[0].cpu().numpy()
    black = (rgba[..., :3] == 0).all(axis=-1) & (rgba[..., 3] == 255)
    assert (black == np.isin(owner, big[:5])).all(), f"{int(black.sum())} black pixels, the five faces own {int(np.isin(owner, big[:5]).sum())}"
    assert (depth[black] > 0).all()


# ---------------------------------------------------------------------------------------------- 7. against the coloured renderer
def test_a_constant_texture_equals_the_coloured_renderer():
    from gigapose_amd import render, texture

    colour = (37, 201, 114)
    v, f, uv = meshes.uv_icosphere(2, 1.0)
    rs = np.random.RandomState(21)
    poses = np.stack([pose(rotation(rs), (0.1, 0.0, d)) for d in (2.0, 5.0, 25.0)] + [pose(np.eye(3), (0, 0, -4.0))]).astype(np.float32)
    args = (_t(v), _t(f))
    want = render.MeshRenderer(240, 320, K_SMALL, ZNEAR)(*args, None, _t(poses), colour=colour, on_clipped="ignore")
    got = texture.TexturedMeshRenderer(240, 320, K_SMALL, ZNEAR)(*args, _t(uv), _t(tr.constant_texture(5, 7, colour)), _t(poses), on_clipped="ignore")
    for key in ("rgba", "depth", "clipped"):
        assert_bits(got[key], want[key], key)
    assert got["clipped"].tolist() == [0, 0, 0, len(f)] and int((got["rgba"][..., 3] == 255).sum()) > 10000
    with pytest.raises(ValueError, match=r"view 3 drops 320 of 320 triangles"):
        texture.TexturedMeshRenderer(240, 320, K_SMALL, ZNEAR)(*args, _t(uv), _t(tr.constant_texture(5, 7, colour)), _t(poses))


# ---------------------------------------------------------------------------------------------- 8. addressing past 2^31
def test_views_past_2_to_31_bytes():
    """875 views at 480 x 640 in ONE call: the key buffer is 2.15 GB, so the last views lie past a 32-bit byte offset.  Views 0
    and 874 show a textured quad and equal the restatement; the views between look past it and are empty."""
    from gigapose_amd import texture

    N, H, W = 875, 480, 640
    assert N * H * W * 8 > 2 ** 31
    v, f, uv = meshes.uv_quad((60.0, 40.0), uv_min=(-0.25, 0.0), uv_max=(1.5, 1.0))
    rs = np.random.RandomState(31)
    poses = np.tile(pose(np.eye(3), (5000.0, 0.0, 300.0)), (N, 1, 1))          # far to the right of the frame, not clipped
    poses[0] = pose(rotation(rs), (5.0, -3.0, 150.0))
    poses[N - 1] = pose(rotation(rs), (-20.0, 12.0, 420.0))
    poses = poses.astype(np.float32)
    tex = tr.noise_texture(64, 64, seed=6)
    out = texture.TexturedMeshRenderer()(_t(v), _t(f), _t(uv), _t(tex), _t(poses), views_per_call=N)
    want = tr.render(v, f, uv, tex, poses[[0, N - 1]], syn.TEMPLATE_K, H, W, 1e-3)
    assert_bits(out["rgba"][[0, N - 1]], want["rgba"], "rgba of the first and the last view")
    assert_bits(out["depth"][[0, N - 1]], want["depth"], "depth of the first and the last view")
    assert int(out["clipped"].abs().sum()) == 0 and (want["rgba"][..., 3] == 255).sum(axis=(1, 2)).min() > 500
    assert int(out["rgba"][400].max()) == 0 and float(out["depth"][400].abs().max()) == 0.0
    assert int(out["rgba"][1:N - 1].max()) == 0
    del out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 9. through the model
def test_textured_templates_through_the_model(tmp_path):
    """The UV box with the quadrant card at 12 views.  Route A: TexturedMeshTemplates (rendered and cropped on the device).  Route
    B: RenderedTemplates on the PNGs save_renders wrote of the same views.  Banks are equal tensor for tensor and so are the
    predictions.  The first three views look straight at the -z, -y and -x faces, which BOX_ATLAS puts into the bottom-left,
    bottom-right and top-left quadrants of the texture: the pixel at the principal point has that quadrant's colour."""
    from gigapose_amd import render, texture
    from gigapose_amd.onboard import RenderedTemplates

    v, f, uv = meshes.uv_box((1.0, 0.8, 0.6))
    card = tr.quadrant_card(64, 64)
    rs = np.random.RandomState(1213)
    to_minus_y = np.asarray([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)      # object -y -> camera -z: that face looks at the camera
    to_minus_x = np.asarray([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float64)
    assert np.allclose(to_minus_y @ (0, -1, 0), (0, 0, -1)) and np.allclose(to_minus_x @ (-1, 0, 0), (0, 0, -1))
    poses = [pose(R, (0.0, 0.0, 5.0)) for R in (np.eye(3), to_minus_y, to_minus_x)]
    poses += [pose(rotation(rs), (rs.uniform(-.3, .3), rs.uniform(-.2, .2), rs.uniform(4.6, 5.4))) for _ in range(9)]
    poses = np.stack(poses).astype(np.float32)
    mesh = dict(vertices=v, faces=f, corner_uv=uv, colours=np.full((len(v), 3), 9, np.uint8))      # the colours are ignored
    mesh_set = texture.TexturedMeshTemplates([(mesh, card, poses)], K=K_SMALL, device=DEV, H=240, W=320, znear=ZNEAR)
    drawn = mesh_set.render(0)
    assert drawn["rgba"].is_cuda and drawn["rgba"].shape == (12, 240, 320, 4)
    for n, quadrant in enumerate(("bottom_left", "bottom_right", "top_left")):
        assert drawn["rgba"][n, 120, 160].tolist() == list(tr.QUADRANTS[quadrant]) + [255], f"view {n}: {drawn['rgba'][n, 120, 160].tolist()}"
    render.save_renders(tmp_path, drawn["rgba"], drawn["depth"], depth_scale=1000.0)
    png_set = RenderedTemplates([(str(tmp_path), poses)], K=K_SMALL, device=DEV)
    item = mesh_set[0]
    assert item.rgb.is_cuda and item.rgb.shape == (12, 3, 224, 224) and item.mask.shape == (12, 224, 224) and item.poses.shape == (12, 4, 4)
    assert_bits(item.K, K_SMALL, "K")
    model = factory.build_model("dinov2_vits14", k=4, device=DEV, seed=70, numerics="chain")
    syn.condition_ist(model.ist_net)
    tar_K, tar_M = syn.crop_geometry(78, 12)
    labels = torch.ones(12, dtype=torch.int64)
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
        assert_bits(banks[0][key], banks[1][key], f"bank: {key}")
    for key in preds[0]:
        assert_bits(preds[0][key], preds[1][key], f"prediction: {key}")
