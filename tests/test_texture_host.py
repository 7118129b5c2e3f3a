"""CPU: the host half of gigapose_amd.texture -- libgigapose_texture.so against include/gigapose_texture.h, argument validation
without a GPU, the loaders -- and the numpy restatement (gigapose_testing/texture_ref.py) against truth that does not go through
it: 2 x 2 means, exact rational arithmetic for the perspective-correct UVs and the level of detail, linear ramps.  The same
comparisons are then run on six deliberately wrong renderers and must reject each."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gigapose_amd import _lib, ingest, onboard, render, rle_strings, texture
from gigapose_testing import meshes, raster_ref
from gigapose_testing import texture_ref as tr
from gigapose_testing.symbols import exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpt_abi_version", "gpt_build_mips", "gpt_last_error", "gpt_mip_levels", "gpt_mip_texels", "gpt_resolve"]


# ---------------------------------------------------------------------------------------------- the library and its header
def test_texture_library_exports_exactly_its_header_and_no_symbol_of_the_other_libraries():
    src = open(os.path.join(ROOT, "include", "gigapose_texture.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(gpt_[a-z0-9_]+)\s*\(", src)))
    assert names == NAMES
    exported = exported_symbols(texture.TEXTURE_LIB_PATH)
    assert [n for n in exported if n.startswith("gpt_")] == names
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the texture library"
    lib = texture.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gpt_abi_version() >= 1
    assert f"{texture.MAX_UV:.1f}f" in src and str(texture.MAX_TEXTURE) in src and tr.MAX_UV == texture.MAX_UV


def test_the_other_libraries_carry_no_texture_symbol():
    paths = (_lib.LIB_PATH, _lib.PROBE_LIB_PATH, ingest.INGEST_LIB_PATH, rle_strings.RLESTR_LIB_PATH, onboard.ONBOARD_LIB_PATH,
             render.RENDER_LIB_PATH)
    assert len(set(paths)) == 6
    for path in paths:
        assert not [n for n in exported_symbols(path) if n.startswith("gpt_")], path


def test_texture_argument_validation_needs_no_gpu():
    lib = texture.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    err = lib.gpt_last_error

    def resolve(vis=one, xy=one, depth=one, V=5, faces=one, F=3, uv=one, pyr=one, Ht=8, Wt=8, N=2, H=48, W=64, rgba=one, z=one):
        return lib.gpt_resolve(vis, xy, depth, V, faces, F, uv, pyr, Ht, Wt, N, H, W, rgba, z, null)

    assert lib.gpt_build_mips(null, 8, 8, one, null) == -1
    assert b"gpt_build_mips" in err() and b"null" in err()
    assert lib.gpt_build_mips(one, 8, 8, null, null) == -1
    assert b"gpt_build_mips" in err() and b"null" in err()
    for Ht, Wt in ((0, 8), (8, 0), (-1, 8), (8, -4), (16385, 8), (8, 16385)):
        assert lib.gpt_build_mips(one, Ht, Wt, one, null) == -1, (Ht, Wt)
        assert b"gpt_build_mips" in err() and b"bad sizes" in err()
        assert resolve(Ht=Ht, Wt=Wt) == -1, (Ht, Wt)
        assert b"gpt_resolve" in err() and b"bad sizes" in err()
    assert lib.gpt_build_mips(one, 8, 8, ctypes.c_void_p(10), null) == -1
    assert b"gpt_build_mips" in err() and b"aligned" in err()

    for kw in (dict(vis=null), dict(xy=null), dict(depth=null), dict(faces=null), dict(uv=null), dict(pyr=null), dict(rgba=null), dict(z=null)):
        assert resolve(**kw) == -1, kw
        assert b"gpt_resolve" in err() and b"null" in err(), kw
    for kw in (dict(V=-5), dict(F=-3), dict(N=-2), dict(H=0), dict(W=-64), dict(H=65536, W=32768), dict(N=65536)):
        assert resolve(**kw) == -1, kw
        assert b"gpt_resolve" in err() and b"bad sizes" in err(), kw
    assert resolve(rgba=ctypes.c_void_p(6)) == -1
    assert b"gpt_resolve" in err() and b"aligned" in err()
    assert resolve(pyr=ctypes.c_void_p(18)) == -1
    assert b"gpt_resolve" in err() and b"aligned" in err()
    assert resolve(vis=null, xy=null, depth=null, faces=null, uv=null, pyr=null, rgba=null, z=null, N=0) == 0    # N = 0: nothing to do
    assert resolve(N=0, Ht=0) == -1                                                                              # ... but still checked


@pytest.mark.parametrize("size", [(1, 1), (1, 256), (5, 7), (64, 64), (16384, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mip_layout_agrees_with_the_restatement(size):
    Ht, Wt = size
    sizes = tr.mip_sizes(Ht, Wt)
    assert sizes[0] == (Ht, Wt) and sizes[-1] == (1, 1) and len(sizes) == 1 + int(np.floor(np.log2(max(Ht, Wt))))
    assert texture.mip_levels(Ht, Wt) == len(sizes) == tr.mip_levels(Ht, Wt)
    assert texture.mip_texels(Ht, Wt) == sum(h * w for h, w in sizes) == tr.mip_texels(Ht, Wt)
    for bad in ((0, 4), (4, 0), (16385, 1), (-3, 3)):
        assert texture.mip_levels(*bad) == 0 and texture.mip_texels(*bad) == 0 and tr.mip_levels(*bad) == 0


# ---------------------------------------------------------------------------------------------- the restatement against truth
# Every check takes the keyword switches of texture_ref (CONTRACT = none) and raises AssertionError when the renderer they select
# is not the contract: the mutants below go through the same code.
def check_pyramid(**variant):
    """A 64 x 32 noise texture: level l+1 is exactly (sum of the 2 x 2 block + 2) >> 2 of level l, within 1/2 (one rounding) of the
    block's float mean, and within l / 2 of the float mean of the 2^l x 2^l block of the image (l roundings, each averaged down).
    Sizes at 5 x 7 and 129 x 257 halve with floor, as the library's gpt_mip_texels says."""
    rounding = variant.get("rounding", "floor")
    for Ht, Wt in ((5, 7), (129, 257), (64, 32)):
        assert sum(h * w for h, w in tr.mip_sizes(Ht, Wt, rounding)) == texture.mip_texels(Ht, Wt), f"{Ht} x {Wt}: texel count"
    rgb = tr.noise_texture(64, 32, seed=4)
    levels = tr.split_levels(tr.build_mips(rgb, rounding), 64, 32, rounding)
    assert (levels[0][..., :3] == rgb).all() and all((lev[..., 3] == 255).all() for lev in levels)
    chain = rgb.astype(np.float64)
    for l in range(1, len(levels)):
        prev = levels[l - 1][..., :3].astype(np.int64)
        if prev.shape[1] == 1:                                      # a dimension has reached 1: the clamp reads it twice
            prev, chain = np.repeat(prev, 2, axis=1), np.repeat(chain, 2, axis=1)
        h, w = prev.shape[:2]
        blocks = prev.reshape(h // 2, 2, w // 2, 2, 3)
        assert levels[l].shape[:2] == blocks.shape[0:3:2], f"level {l}"
        assert (levels[l][..., :3] == (blocks.sum(axis=(1, 3)) + 2) >> 2).all(), f"level {l}"
        assert np.abs(levels[l][..., :3] - blocks.mean(axis=(1, 3))).max() <= 0.5
        chain = chain.reshape(h // 2, 2, w // 2, 2, 3).mean(axis=(1, 3))
        assert np.abs(levels[l][..., :3] - chain).max() <= 0.5 * l, f"level {l} against the float chain"
    assert len(levels) == 7 and levels[5].shape[:2] == (2, 1) and levels[6].shape[:2] == (1, 1)


TRIANGLES = {   # screen coordinates in 1/256 pixel (not on pixel centres), f32 depths, corner UVs
    "frontal": ([(3 * 256 + 17, 2 * 256 + 5), (60 * 256 + 100, 5 * 256 + 9), (20 * 256 + 33, 45 * 256 + 77)], [2.0, 2.0, 2.0]),
    "grazing": ([(3 * 256 + 17, 2 * 256 + 5), (60 * 256 + 100, 5 * 256 + 9), (20 * 256 + 33, 45 * 256 + 77)], [1.0, 30.0, 7.5]),
    "negative area": ([(3 * 256 + 17, 2 * 256 + 5), (20 * 256 + 33, 45 * 256 + 77), (60 * 256 + 100, 5 * 256 + 9)], [1.0, 7.5, 30.0]),
}
TRI_UV = np.asarray([[(0.21, 0.33), (0.87, 0.42), (0.35, 0.91)]], np.float32)
TRI_H, TRI_W, TRI_TEX = 48, 64, (512, 384)


def exact_pixel(pts, depth, uv, x, y, Ht, Wt):
    """(u, v, rho2, l0) of pixel (x, y) in exact rational arithmetic, from the definition (no incremental edge values)."""
    area = (pts[1][0] - pts[0][0]) * (pts[2][1] - pts[0][1]) - (pts[1][1] - pts[0][1]) * (pts[2][0] - pts[0][0])
    order = (0, 1, 2) if area > 0 else (0, 2, 1)
    p = [pts[k] for k in order]
    r = [1 / Fraction(float(depth[k])) for k in order]
    cu = [Fraction(float(uv[k][0])) for k in order]
    cv = [Fraction(float(uv[k][1])) for k in order]

    def at(X, Y):
        e = [(p[b][0] - p[a][0]) * (Y - p[a][1]) - (p[b][1] - p[a][1]) * (X - p[a][0]) for a, b in ((1, 2), (2, 0), (0, 1))]
        t = [e[k] * r[k] for k in range(3)]
        q = sum(t)
        return q, sum(t[k] * cu[k] for k in range(3)) / q, sum(t[k] * cv[k] for k in range(3)) / q

    q, u, v = at(256 * x, 256 * y)
    qx, ux, vx = at(256 * (x + 1), 256 * y)
    qy, uy, vy = at(256 * x, 256 * (y + 1))
    top = tr.mip_levels(Ht, Wt) - 1
    rho2 = max(((ux - u) * Wt) ** 2 + ((vx - v) * Ht) ** 2, ((uy - u) * Wt) ** 2 + ((vy - v) * Ht) ** 2)
    if qx <= 0 or qy <= 0:
        return u, v, None, top
    l0 = 0
    while l0 < top and 4 ** (l0 + 1) <= rho2:
        l0 += 1
    return u, v, rho2, l0


def check_uv_and_level(**variant):
    """Three triangles, <= 200 sampled pixels in all: float64 (u, v) of the restatement agree with the exact values to 1e-12
    relative, l0 equals the exact level wherever the exact rho2 is not within 1e-9 relative of a power of 4."""
    Ht, Wt = TRI_TEX
    faces = np.asarray([(0, 1, 2)], np.int32)
    checked, levels = 0, set()
    for name, (pts, depth) in TRIANGLES.items():
        xy, z = np.asarray([pts], np.int32), np.asarray([depth], np.float32)
        vis, _ = raster_ref.raster(xy, z, faces, TRI_H, TRI_W)
        info = tr.inspect(vis, xy, z, faces, TRI_UV, Ht, Wt, **variant)
        ys, xs = np.nonzero(info["covered"][0])
        assert len(ys) > 500, name
        pick = np.random.RandomState(len(name)).choice(len(ys), 66, replace=False)
        for y, x in zip(ys[pick], xs[pick]):
            u, v, rho2, l0 = exact_pixel(pts, depth, TRI_UV[0], int(x), int(y), Ht, Wt)
            got_u, got_v = Fraction(float(info["u"][0, y, x])), Fraction(float(info["v"][0, y, x]))
            assert abs(got_u - u) <= Fraction(1, 10 ** 12) * abs(u), f"{name}: u at ({x}, {y}): {float(got_u)} vs {float(u)}"
            assert abs(got_v - v) <= Fraction(1, 10 ** 12) * abs(v), f"{name}: v at ({x}, {y}): {float(got_v)} vs {float(v)}"
            near = rho2 is not None and rho2 >= 1 and any(abs(rho2 - 4 ** k) <= Fraction(1, 10 ** 9) * 4 ** k for k in range(16))
            if not near:
                assert int(info["l0"][0, y, x]) == l0, f"{name}: level at ({x}, {y}): {info['l0'][0, y, x]} vs {l0}, rho2 = {float(rho2 or 0)}"
                if rho2 is not None and 1 <= rho2 < 4 ** l0 * 4:
                    w = float((rho2 / 4 ** l0 - 1) / 3)
                    assert abs(info["w"][0, y, x] - w) <= 1e-9, f"{name}: weight at ({x}, {y})"
                levels.add(l0)
            checked += 1
    assert 150 <= checked <= 200 and len(levels) >= 3 and max(levels) >= 2, (checked, levels)


def frontal_quad(H, W, uv_min, uv_max):
    """A quad that fills the frame's middle, seen head-on at depth 4 with a 256 px focal length: one view's keys and the rest."""
    v, f, uv = meshes.uv_quad((0.75, 0.5), uv_min=uv_min, uv_max=uv_max)          # 48 x 32 pixels
    K = np.asarray([256, 0, (W - 1) / 2, 0, 256, (H - 1) / 2, 0, 0, 1], np.float32)
    P = np.eye(4, dtype=np.float32)[None].copy()
    P[0, 2, 3] = 4.0
    xy, z = raster_ref.project(v, P, K, 1e-3)
    vis, clipped = raster_ref.raster(xy, z, f, H, W)
    assert clipped.tolist() == [0]
    return vis, xy, z, f, uv


def check_ramps(**variant):
    """Magnified ramps (8 texels over 48 or 32 pixels: level 0 alone).  The ideal texture is c(x) = 255 x / 7 at texel centre x,
    continued periodically; bilinear filtering of the rounded texels is within 1/2 + 1/2 of the piecewise-linear function through
    the ideal texels.  The u ramp is drawn with u in [-0.5, 1.5] (repeat: the ramp starts again); the v ramp with v in [0, 1]."""
    H, W = 40, 64
    for axis, (lo, hi) in (("u", ((-0.5, 0.0), (1.5, 1.0))), ("v", ((0.0, 0.0), (1.0, 1.0)))):
        vis, xy, z, f, uv = frontal_quad(H, W, lo, hi)
        tex = tr.ramp_u(4, 8) if axis == "u" else tr.ramp_v(8, 4)
        Ht, Wt = tex.shape[:2]
        truth = tr.inspect(vis, xy, z, f, uv, Ht, Wt)                # u, v of the contract (held to exact arithmetic above)
        rgba, _ = tr.resolve(vis, xy, z, f, uv, tr.build_mips(tex, variant.get("rounding", "floor")), Ht, Wt, **variant)
        c = truth["covered"][0]
        assert c.sum() == 48 * 32 and (truth["l0"][0][c] == 0).all() and not truth["two"][0][c].any()
        coord = truth["u"][0][c] if axis == "u" else truth["v"][0][c]
        s = (coord * 8 - 0.5) % 8.0                                 # position in texel units, periodic; v = 0 is the dark bottom row
        k = np.floor(s)
        ideal = (255.0 / 7.0) * (k * (1 - (s - k)) + ((k + 1) % 8) * (s - k))
        got = rgba[0][c].astype(np.float64)
        assert (got[:, 3] == 255).all() and (got[:, 0] == got[:, 1]).all() and (got[:, 1] == got[:, 2]).all()
        assert np.abs(got[:, 0] - ideal).max() <= 1.0, f"{axis} ramp: {np.abs(got[:, 0] - ideal).max():.2f} LSB from the linear function"
        assert got[:, 0].min() <= 10 and got[:, 0].max() >= 245           # the whole ramp was looked at


def test_restatement_pyramid_is_the_rounded_2x2_mean():
    check_pyramid()


def test_restatement_uv_and_level_against_exact_rational_arithmetic():
    check_uv_and_level()


def test_restatement_ramps_are_linear_and_repeat():
    check_ramps()


def test_a_constant_texture_gives_that_constant_for_every_uv_and_level():
    """The UV icosphere (UVs from 0.03 to 1.09: wrap) at three distances with a 5 x 7 texture of one colour, and a quad whose UVs
    run from -3 to 40: every level of detail occurs, and every covered pixel is the colour."""
    colour = (201, 7, 98)
    tex = tr.constant_texture(5, 7, colour)
    v, f, uv = meshes.uv_icosphere(1, 1.0)
    K = np.asarray([60, 0, 31.5, 0, 60, 23.5, 0, 0, 1], np.float32)
    seen = set()
    for dist in (2.5, 9.0, 40.0):
        P = np.eye(4, dtype=np.float32)[None].copy()
        P[0, :3, 3] = (0.1, -0.05, dist)
        out = tr.render(v, f, uv, tex, P, K, 48, 64, 1e-3)
        info = tr.inspect(out["vis"], out["xy"], out["vdepth"], f, uv, 5, 7)
        a = out["rgba"][0][..., 3] == 255
        assert a.sum() >= 4 and (out["rgba"][0][a][:, :3] == colour).all() and (out["rgba"][0][~a] == 0).all()
        seen |= set(zip(info["l0"][0][a].tolist(), info["two"][0][a].tolist()))
    vis, xy, z, f, uv = frontal_quad(40, 64, (-3.0, -3.0), (40.0, 40.0))
    rgba, _ = tr.resolve(vis, xy, z, f, uv, tr.build_mips(tex), 5, 7)
    assert (rgba[0][vis[0] != raster_ref.EMPTY_KEY][:, :3] == colour).all()
    info = tr.inspect(vis, xy, z, f, uv, 5, 7)
    seen |= set(zip(info["l0"][0][info["covered"][0]].tolist(), info["two"][0][info["covered"][0]].tolist()))
    assert {(0, False), (0, True), (1, True), (2, False)} <= seen, seen


MUTANTS = {"affine interpolation": (dict(interp="affine"), check_uv_and_level),
           "corner UVs not swapped on negative area": (dict(swap_uv=False), check_uv_and_level),
           "v not flipped": (dict(flip_v=False), check_ramps),
           "clamp in place of repeat": (dict(wrap="clamp"), check_ramps),
           "l0 one too low": (dict(l0_shift=-1), check_uv_and_level),
           "level sizes by ceiling": (dict(rounding="ceil"), check_pyramid)}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_checks_reject_wrong_renderers(name):
    variant, check = MUTANTS[name]
    assert set(variant) <= set(tr.CONTRACT) and all(tr.CONTRACT[k] != val for k, val in variant.items())
    with pytest.raises(AssertionError):
        check(**variant)
    check(**{k: tr.CONTRACT[k] for k in variant})                   # the same switch at its contract value passes


# ---------------------------------------------------------------------------------------------- loaders
def write_textured_ply(path, fmt, v, f, vertex_uv=None, names=("texture_u", "texture_v"), face_uv=None, texnumber=None, comment=None,
                       colours=None):
    vprops = [(k, "f4", v[:, j]) for j, k in enumerate("xyz")]
    if colours is not None:
        vprops += [(k, "u1", colours[:, j]) for j, k in enumerate(("red", "green", "blue"))]
    if vertex_uv is not None:
        vprops += [(names[0], "f4", vertex_uv[:, 0]), (names[1], "f4", vertex_uv[:, 1])]
    ply = {"f4": "float", "u1": "uchar"}
    head = ["ply", f"format {fmt} 1.0", "comment written by the test"] + ([f"comment TextureFile {comment}"] if comment else [])
    head += [f"element vertex {len(v)}"] + [f"property {ply[t]} {k}" for k, t, _ in vprops]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    head += ["property list uchar float texcoord"] if face_uv is not None else []
    head += ["property int texnumber"] if texnumber is not None else []
    head += ["end_header"]
    if fmt == "ascii":
        lines = [" ".join(repr(float(a[i])) if t[0] == "f" else str(int(a[i])) for _, t, a in vprops) for i in range(len(v))]
        for i, row in enumerate(f):
            w = ["3"] + [str(int(k)) for k in row]
            if face_uv is not None:
                w += [str(len(face_uv[i]))] + [repr(float(x)) for x in face_uv[i]]
            if texnumber is not None:
                w += [str(int(texnumber[i]))]
            lines.append(" ".join(w))
        body = ("\n".join(lines) + "\n").encode()
    else:
        rec = np.zeros(len(v), np.dtype([(k, "<" + t) for k, t, _ in vprops]))
        for k, _, a in vprops:
            rec[k] = a
        body = rec.tobytes()
        for i, row in enumerate(f):
            body += np.asarray([3], "<u1").tobytes() + np.asarray(row, "<i4").tobytes()
            if face_uv is not None:
                body += np.asarray([len(face_uv[i])], "<u1").tobytes() + np.asarray(face_uv[i], "<f4").tobytes()
            if texnumber is not None:
                body += np.asarray([texnumber[i]], "<i4").tobytes()
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode() + body)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_load_textured_ply(tmp_path, fmt):
    v, f, corner = meshes.uv_box((1.0, 0.6, 0.3), shared=False)
    v = (v + np.float32(0.123456789)).astype(np.float32)
    rs = np.random.RandomState(9)
    vertex_uv = rs.uniform(-0.5, 1.5, (len(v), 2)).astype(np.float32)
    colours = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    path = str(tmp_path / "m.ply")

    def same_mesh(m, c=None):
        assert sorted(m) == ["colours", "corner_uv", "faces", "texture_file", "vertices"]
        np.testing.assert_array_equal(m["vertices"], v)
        np.testing.assert_array_equal(m["faces"], f)
        assert m["corner_uv"].dtype == np.float32 and m["corner_uv"].shape == (len(f), 3, 2)
        assert (m["colours"] is None) if c is None else (m["colours"] == c).all()
        got = render.load_ply(path)                                   # load_ply on the same file: a 3-tuple, unchanged
        assert isinstance(got, tuple) and len(got) == 3
        np.testing.assert_array_equal(got[0], v)
        np.testing.assert_array_equal(got[1], f)
        assert (got[2] is None) if c is None else (got[2] == c).all()

    for names in (("texture_u", "texture_v"), ("u", "v"), ("s", "t")):
        write_textured_ply(path, fmt, v, f, vertex_uv=vertex_uv, names=names)
        m = texture.load_textured_ply(path)
        same_mesh(m)
        np.testing.assert_array_equal(m["corner_uv"], vertex_uv[f])
        assert m["texture_file"] is None
    face_uv = corner.reshape(len(f), 6)
    write_textured_ply(path, fmt, v, f, face_uv=face_uv, texnumber=np.zeros(len(f), np.int32), comment="obj_000007.png", colours=colours)
    m = texture.load_textured_ply(path)
    same_mesh(m, colours)
    np.testing.assert_array_equal(m["corner_uv"], corner)
    assert m["texture_file"] == "obj_000007.png"
    write_textured_ply(path, fmt, v, f, vertex_uv=vertex_uv, face_uv=face_uv, comment="a b.png")      # both: the per-face form wins
    m = texture.load_textured_ply(path)
    same_mesh(m)
    np.testing.assert_array_equal(m["corner_uv"], corner)
    assert m["texture_file"] == "a b.png"
    np.testing.assert_array_equal(texture.corner_uv_from_vertices(vertex_uv, f), vertex_uv[f])

    tn = np.zeros(len(f), np.int32)
    tn[5] = 1
    write_textured_ply(path, fmt, v, f, face_uv=face_uv, texnumber=tn)
    with pytest.raises(ValueError, match="texnumber != 0: several textures per model are out of scope"):
        texture.load_textured_ply(path)
    short = [list(r) for r in face_uv]
    short[3] = short[3][:5]
    write_textured_ply(path, fmt, v, f, face_uv=short)
    with pytest.raises(ValueError, match="does not hold six values"):
        texture.load_textured_ply(path)
    write_textured_ply(path, fmt, v, f, face_uv=[r[:5] for r in short])                              # every list too short
    with pytest.raises(ValueError, match="does not hold six values"):
        texture.load_textured_ply(path)
    write_textured_ply(path, fmt, v, f, colours=colours)
    with pytest.raises(ValueError, match="no texture coordinates"):
        texture.load_textured_ply(path)
    assert len(render.load_ply(path)) == 3


def test_load_texture(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(2)
    rgb = rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    Image.fromarray(rgb, "RGB").save(str(tmp_path / "rgb.png"))
    got = texture.load_texture(tmp_path / "rgb.png")
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(got, rgb)
    rgba = np.concatenate([rgb, rs.randint(0, 256, (5, 7, 1)).astype(np.uint8)], axis=2)
    Image.fromarray(rgba, "RGBA").save(str(tmp_path / "rgba.png"))
    np.testing.assert_array_equal(texture.load_texture(str(tmp_path / "rgba.png")), rgb)               # alpha is dropped
    Image.fromarray(rgb[..., 0], "L").save(str(tmp_path / "grey.png"))
    np.testing.assert_array_equal(texture.load_texture(str(tmp_path / "grey.png")), np.repeat(rgb[..., :1], 3, axis=2))
    pal = Image.fromarray(rgb, "RGB").quantize(colors=16)
    assert pal.mode == "P"
    pal.save(str(tmp_path / "pal.png"))
    np.testing.assert_array_equal(texture.load_texture(str(tmp_path / "pal.png")), np.asarray(pal.convert("RGB")))
    Image.fromarray(rs.randint(0, 65536, (5, 7)).astype(np.uint16)).save(str(tmp_path / "deep.png"))
    with pytest.raises(ValueError, match="16-bit"):
        texture.load_texture(str(tmp_path / "deep.png"))


# ---------------------------------------------------------------------------------------------- validation in Python
def test_cpu_input_has_no_fallback_and_wrong_shapes_are_rejected(tmp_path):
    import torch

    v, f, uv = meshes.uv_box()
    tex = tr.quadrant_card(8, 8)
    poses = np.eye(4, dtype=np.float32)[None]
    tv, tf, tuv, tt, tp = (torch.from_numpy(np.ascontiguousarray(a)) for a in (v, f, uv, tex, poses))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        texture.TexturedMeshRenderer(48, 64)(tv, tf, tuv, tt, tp)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        texture.build_mips(tt)
    mesh = dict(vertices=v, faces=f, corner_uv=uv)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        texture.TexturedMeshTemplates([(mesh, tex, poses)], device="cpu")[0]
    with pytest.raises(ValueError, match="on_clipped"):
        texture.TexturedMeshRenderer(48, 64)(tv, tf, tuv, tt, tp, on_clipped="warn")
    for bad, what in ((dict(mesh, corner_uv=uv[:-1]), "corner_uv"), (dict(mesh, corner_uv=uv.reshape(-1, 6)), "corner_uv"),
                      (dict(mesh, vertices=v[:, :2]), "vertices"), (dict(mesh, faces=f + 1), "face index is outside"),
                      ((v, f, uv), "dict with vertices, faces and corner_uv")):
        with pytest.raises(ValueError, match=what):
            texture.TexturedMeshTemplates([(bad, tex, poses)], device="cpu")
    for bad_tex in (tex[..., 0], tex[:, :, :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="expected a texture"):
            texture.TexturedMeshTemplates([(mesh, bad_tex, poses)], device="cpu")
    with pytest.raises(ValueError, match=r"expected poses \(N, 4, 4\)"):
        texture.TexturedMeshTemplates([(mesh, tex, np.eye(4))], device="cpu")
    with pytest.raises(ValueError, match="names none"):
        texture.TexturedMeshTemplates([(mesh, None, poses)], device="cpu")
    with pytest.raises(ValueError, match=r"expected \(mesh, texture, poses\)"):
        texture.TexturedMeshTemplates([(mesh, poses)], device="cpu")
    # a PLY with `comment TextureFile`: texture=None takes the file next to it
    Image = pytest.importorskip("PIL.Image")
    Image.fromarray(tex, "RGB").save(str(tmp_path / "card.png"))
    write_textured_ply(str(tmp_path / "m.ply"), "ascii", v, f, face_uv=uv.reshape(len(f), 6), comment="card.png")
    ds = texture.TexturedMeshTemplates([(str(tmp_path / "m.ply"), None, poses), (str(tmp_path / "m.ply"), tex[::-1].copy(), poses)], device="cpu")
    assert len(ds) == 2
    np.testing.assert_array_equal(ds._meshes[0][3].numpy(), tex)
    np.testing.assert_array_equal(ds._meshes[1][3].numpy(), tex[::-1])
    np.testing.assert_array_equal(ds._meshes[0][2].numpy(), uv)
