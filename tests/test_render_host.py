"""CPU: the host half of gigapose_amd.render -- libgigapose_render.so against include/gigapose_render.h, argument validation
without a GPU, load_ply, save_renders -> load_renders -- and the coverage rule of the numpy restatement
(gigapose_testing/raster_ref.py): it partitions a convex polygon whatever the triangulation and the winding, and the same check
reports double or missing coverage for rasterisers that are wrong."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gigapose_amd import _lib, ingest, onboard, render
from gigapose_testing import meshes, raster_ref
from gigapose_testing.symbols import exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the library and its header
def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gigapose_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpr_[a-z0-9_]+)\s*\(", src)))


def test_render_library_exports_exactly_its_header_and_no_symbol_of_the_other_libraries():
    names = declared_symbols()
    assert names == ["gpr_abi_version", "gpr_last_error", "gpr_project", "gpr_raster", "gpr_raster_workspace_bytes", "gpr_resolve",
                     "gpr_small_triangle_pixels"]
    exported = exported_symbols(render.RENDER_LIB_PATH)
    assert [n for n in exported if n.startswith("gpr_")] == names
    for prefix in ("gp_", "gpi_", "gpo_", "gps_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the render library"
    lib = render.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gpr_abi_version() >= 1
    assert lib.gpr_small_triangle_pixels() >= 16


def test_the_other_libraries_carry_no_render_symbol():
    for path in (_lib.LIB_PATH, _lib.PROBE_LIB_PATH, ingest.INGEST_LIB_PATH, onboard.ONBOARD_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert "gpr_" not in out, path


def test_render_argument_validation_needs_no_gpu():
    lib = render.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    K = (ctypes.c_float * 9)(572.0, 0, 320, 0, 573.0, 240, 0, 0, 1)
    zn = ctypes.c_float(0.001)
    err = lib.gpr_last_error
    assert lib.gpr_project(null, 5, null, 2, K, zn, null, null, null) == -1
    assert b"gpr_project" in err() and b"null" in err()
    assert lib.gpr_project(one, -1, one, 2, K, zn, one, one, null) == -1                      # negative count
    assert b"gpr_project" in err() and b"bad sizes" in err()
    assert lib.gpr_project(one, 5, one, 65536, K, zn, one, one, null) == -1                   # N > 65535
    assert lib.gpr_project(one, 5, one, 2, K, ctypes.c_float(0.0), one, one, null) == -1
    assert b"znear" in err()
    assert lib.gpr_project(one, 5, one, 2, K, ctypes.c_float(float("nan")), one, one, null) == -1
    bad_K = (ctypes.c_float * 9)(572.0, 0, 320, 0, 573.0, 240, 0, 0, 2)
    assert lib.gpr_project(one, 5, one, 2, bad_K, zn, one, one, null) == -1
    assert b"last row of K" in err()
    assert lib.gpr_project(null, 5, null, 0, K, zn, null, null, null) == 0                    # N = 0: nothing to do

    assert lib.gpr_raster(null, null, 5, null, 3, 2, 48, 64, null, null, null, null) == -1
    assert b"gpr_raster" in err() and b"null" in err()
    assert lib.gpr_raster(one, one, 5, null, 3, 2, 48, 64, one, one, one, null) == -1         # faces null, before anything is enqueued
    assert b"null" in err()
    assert lib.gpr_raster(one, one, 5, one, 3, 2, 65536, 65536, one, one, one, null) == -1    # H*W >= 2^31
    assert b"gpr_raster" in err() and b"bad sizes" in err()
    assert lib.gpr_raster(one, one, 5, one, -3, 2, 48, 64, one, one, one, null) == -1
    assert lib.gpr_raster(one, one, -5, one, 3, 2, 48, 64, one, one, one, null) == -1
    assert lib.gpr_raster(one, one, 5, one, 3, -2, 48, 64, one, one, one, null) == -1
    assert lib.gpr_raster(one, one, 5, one, 3, 2, 0, 64, one, one, one, null) == -1
    assert lib.gpr_raster(one, one, 5, one, 3, 2, 48, 64, ctypes.c_void_p(12), one, one, null) == -1
    assert b"aligned" in err()
    assert lib.gpr_raster(null, null, 5, null, 3, 0, 48, 64, null, null, null, null) == 0

    assert lib.gpr_resolve(null, null, null, 5, null, 3, null, 2, 48, 64, null, null, null) == -1
    assert b"gpr_resolve" in err() and b"null" in err()
    assert lib.gpr_resolve(one, one, one, 5, one, 3, one, 2, 65536, 32768, one, one, null) == -1
    assert b"gpr_resolve" in err() and b"bad sizes" in err()
    assert lib.gpr_resolve(one, one, one, 5, one, 3, one, 65536, 48, 64, one, one, null) == -1
    assert lib.gpr_resolve(one, one, one, 5, one, 3, one, 2, 48, 64, ctypes.c_void_p(6), one, null) == -1
    assert b"aligned" in err()
    assert lib.gpr_resolve(null, null, null, 5, null, 3, null, 0, 48, 64, null, null, null) == 0

    assert lib.gpr_raster_workspace_bytes(162, 20480) >= 162 * 20480 * 8
    assert lib.gpr_raster_workspace_bytes(65535, 2 ** 31 - 1) >= 65535 * (2 ** 31 - 1) * 8          # size_t arithmetic
    assert lib.gpr_raster_workspace_bytes(-1, 5) == 0


def test_cpu_input_has_no_fallback():
    import torch

    v, f, c = (torch.from_numpy(a) for a in meshes.box())
    poses = torch.eye(4)[None]
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        render.MeshRenderer(48, 64)(v, f, c, poses)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        render.MeshTemplates([(meshes.box(), np.eye(4)[None])], device="cpu")[0]
    with pytest.raises(ValueError, match="textures are out of scope"):
        render.MeshTemplates([((v, f, None), np.eye(4)[None])], device="cpu")


def test_template_object_poses_scales_a_copy():
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, :3, 3] = [[0, 0, 1000], [10, -20, 900], [1, 2, 3]]
    out = render.template_object_poses(poses)
    np.testing.assert_array_equal(out[:, :3, 3], poses[:, :3, 3] * 0.4)
    np.testing.assert_array_equal(out[:, :3, :3], poses[:, :3, :3])
    assert poses[0, 2, 3] == 1000
    np.testing.assert_array_equal(render.template_object_poses(poses, zoom=1.0), poses)


# ---------------------------------------------------------------------------------------------- load_ply
_NP2PLY = {"f4": "float", "f8": "double", "u1": "uchar", "i4": "int", "u4": "uint", "i2": "short", "u2": "ushort"}


def write_ply(path, fmt, v, f, c=None, normals=False, alpha=False, count_t="u1", index_t="i4", index_name="vertex_indices", coord_t="f4",
              fmt_line=None, drop_bytes=0):
    props = [(k, coord_t, v[:, j]) for j, k in enumerate("xyz")]
    if normals:
        props += [(k, "f4", np.linspace(-1, 1, len(v)).astype(np.float32) * (j + 1)) for j, k in enumerate(("nx", "ny", "nz"))]
    if c is not None:
        props += [(k, "u1", c[:, j]) for j, k in enumerate(("red", "green", "blue"))]
    if alpha:
        props += [("alpha", "u1", np.full(len(v), 255, np.uint8))]
    props += [("texture_u", "f4", np.zeros(len(v), np.float32))] if normals else []
    head = ["ply", fmt_line or f"format {fmt} 1.0", "comment written by the test", f"element vertex {len(v)}"]
    head += [f"property {_NP2PLY[t]} {k}" for k, t, _ in props]
    head += [f"element face {len(f)}", f"property list {_NP2PLY[count_t]} {_NP2PLY[index_t]} {index_name}", "end_header"]
    body = b""
    if fmt == "ascii":
        lines = [" ".join(repr(float(a[i])) if t[0] == "f" else str(int(a[i])) for _, t, a in props) for i in range(len(v))]
        lines += [" ".join([str(len(row))] + [str(int(i)) for i in row]) for row in f]
        body = ("\n".join(lines) + "\n").encode()
    else:
        rec = np.zeros(len(v), np.dtype([(k, "<" + t) for k, t, _ in props]))
        for k, _, a in props:
            rec[k] = a
        body = rec.tobytes()
        for row in f:
            body += np.asarray([len(row)], "<" + count_t).tobytes() + np.asarray(row, "<" + index_t).tobytes()
    data = ("\n".join(head) + "\n").encode() + body
    with open(path, "wb") as fh:
        fh.write(data[:len(data) - drop_bytes])


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_load_ply_round_trips(tmp_path, fmt):
    v, f, c = meshes.three_boxes(scale=37.5)
    v = (v + np.float32(0.123456789)).astype(np.float32)                      # values that need all their digits
    path = str(tmp_path / "m.ply")
    for kw in (dict(), dict(c=c), dict(c=c, normals=True, alpha=True), dict(c=c, index_t="u4"), dict(index_t="u4", index_name="vertex_index"),
               dict(c=c, count_t="i4", index_t="i2", normals=True), dict(c=c, coord_t="f8", alpha=True)):
        write_ply(path, fmt, v, f, **kw)
        gv, gf, gc = render.load_ply(path)
        assert gv.dtype == np.float32 and gf.dtype == np.int32 and gv.shape == v.shape and gf.shape == f.shape, kw
        np.testing.assert_array_equal(gv, v, err_msg=str(kw))
        np.testing.assert_array_equal(gf, f, err_msg=str(kw))
        if "c" in kw:
            assert gc.dtype == np.uint8
            np.testing.assert_array_equal(gc, c, err_msg=str(kw))
        else:
            assert gc is None, kw


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_load_ply_rejections(tmp_path, fmt):
    v, f, c = meshes.box()
    path = str(tmp_path / "bad.ply")
    quad = [list(r) for r in f[:-2]] + [[0, 1, 2, 3]]
    write_ply(path, fmt, v, quad, c)
    with pytest.raises(ValueError, match="not a triangle"):
        render.load_ply(path)
    mixed = [[0, 1, 2, 3]] + [list(r) for r in f[2:]]                        # the first row sets no pattern the rest follows
    write_ply(path, fmt, v, mixed, c)
    with pytest.raises(ValueError, match="not a triangle"):
        render.load_ply(path)
    far = f.copy()
    far[5, 1] = len(v)
    write_ply(path, fmt, v, far, c)
    with pytest.raises(ValueError, match=r"index is outside \[0, 24\)"):
        render.load_ply(path)
    write_ply(path, fmt, v, f, c, drop_bytes=7)
    with pytest.raises(ValueError, match="truncated"):
        render.load_ply(path)
    write_ply(path, fmt, v[:3], f[:0], c[:3], drop_bytes=20)                  # cut inside the vertex element
    with pytest.raises(ValueError, match="truncated"):
        render.load_ply(path)
    write_ply(path, fmt, v, f, c, fmt_line="format binary_big_endian 1.0")
    with pytest.raises(ValueError, match="binary_big_endian"):
        render.load_ply(path)
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\n")
    with pytest.raises(ValueError, match="truncated"):
        render.load_ply(path)


# ---------------------------------------------------------------------------------------------- the coverage rule
N_POLYGONS = 1500
H, W = 24, 32


def polygon_cases():
    rs = np.random.RandomState(20240)
    for k in range(N_POLYGONS):
        yield k, meshes.screen_polygon(rs, H, W, on_centres=k % 2 == 0)


def fan_counts(p, c, rule):
    """Coverage counts of the four drawings of one polygon: fan about vertex 0 / about the interior point, either winding."""
    out = []
    for pts in (p, p[::-1]):
        n = len(pts)
        xy = np.concatenate([pts, c]).astype(np.int32)
        for about_centre in (False, True):
            out.append(raster_ref.coverage(xy, meshes.fan_faces(n, about_centre), H, W, rule))
    return out


def partition_failures(rule, limit=N_POLYGONS):
    """-> (polygons with a pixel covered twice, polygons where the drawings disagree or a pixel inside is missed)."""
    double = missing = 0
    for k, (p, c) in polygon_cases():
        if k >= limit:
            break
        counts = fan_counts(p, c, rule)
        double += any((cnt > 1).any() for cnt in counts)
        missing += any(((cnt > 0) != (counts[0] > 0)).any() for cnt in counts[1:])
    return double, missing


def test_polygon_generator_is_what_the_test_needs():
    sizes, centred = set(), 0
    for k, (p, c) in polygon_cases():
        sizes.add(len(p))
        on = bool((p % 256 == 0).all())
        assert on or k % 2 == 1                                # the odd cases are off-centre except by chance
        centred += on
        assert np.abs(p).max() < 64 * 256                       # some reach past the frame: the box clamp is part of the check
    assert sizes == set(range(3, 9)) and N_POLYGONS // 2 <= centred < N_POLYGONS // 2 + 10


def test_top_left_rule_partitions_every_convex_polygon():
    """1 500 strictly convex polygons of 3..8 vertices on a 32 x 24 frame, half with every vertex on a pixel centre: the fan about
    vertex 0 and the fan about the snapped centroid, in either winding, cover the same pixels, each exactly once."""
    covered = 0
    for k, (p, c) in polygon_cases():
        counts = fan_counts(p, c, "top_left")
        for j, cnt in enumerate(counts):
            assert cnt.max() <= 1, f"polygon {k}, drawing {j}: a pixel is covered {cnt.max()} times"
            assert (cnt == counts[0]).all(), f"polygon {k}: drawing {j} covers other pixels than drawing 0"
        covered += int(counts[0].sum())
    assert covered > 50 * N_POLYGONS                             # the polygons are not slivers: the check looked at pixels


@pytest.mark.parametrize("rule,kind", [("closed", "double"), ("open", "missing"), ("ties_on_edge0", "either"), ("ties_dx_or_dy", "either")])
def test_the_partition_check_rejects_wrong_rasterisers(rule, kind):
    """e >= 0 on all edges draws shared edges twice; e > 0 alone never draws them; a tie-break on the wrong edges does one or the
    other depending on the direction of the edge.  300 polygons suffice for each to be caught many times."""
    double, missing = partition_failures(rule, limit=300)
    if kind == "double":
        assert double > 100
    elif kind == "missing":
        assert missing > 100 and double == 0
    else:
        assert double + missing > 100
    assert partition_failures("top_left", limit=300) == (0, 0)


def test_restatement_key_order_and_depth():
    """Two coplanar duplicates: the lower face index wins; a nearer triangle wins over both; reversed face list, same depths."""
    xy = np.asarray([[[2 * 256, 2 * 256], [20 * 256, 3 * 256], [5 * 256, 18 * 256], [2 * 256, 2 * 256], [20 * 256, 3 * 256], [5 * 256, 18 * 256],
                      [0, 0], [12 * 256, 0], [0, 12 * 256]]], np.int32)
    depth = np.asarray([[4, 5, 6, 4, 5, 6, 2, 2, 2]], np.float32)
    faces = np.asarray([(0, 1, 2), (3, 4, 5), (6, 7, 8)], np.int32)
    vis, clipped = raster_ref.raster(xy, depth, faces, 24, 32)
    face = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    covered = vis != raster_ref.EMPTY_KEY
    assert clipped.tolist() == [0] and set(np.unique(face[covered])) == {0, 2}
    assert face[0, 3, 3] == 2 and face[0, 10, 8] == 0
    z = (vis >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert z[0, 3, 3] == 2.0 and 4.0 < z[0, 10, 8] < 6.0
    vis_r, _ = raster_ref.raster(xy, depth, faces[::-1].copy(), 24, 32)
    np.testing.assert_array_equal(vis_r >> np.uint64(32), vis >> np.uint64(32))
    colours = np.zeros((9, 3), np.uint8)
    colours[:3], colours[3:6], colours[6:] = (255, 0, 0), (0, 255, 0), (10, 20, 30)
    rgba, zd = raster_ref.resolve(vis, xy, depth, faces, colours)
    assert rgba[0, 10, 8].tolist() == [255, 0, 0, 255] and rgba[0, 3, 3].tolist() == [10, 20, 30, 255]
    assert rgba[0, 23, 31].tolist() == [0, 0, 0, 0] and zd[0, 23, 31] == 0 and zd[0, 3, 3] == 2.0


# ---------------------------------------------------------------------------------------------- save_renders
def test_save_renders_round_trips_through_load_renders(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(5)
    rgba = rs.randint(0, 256, (3, 12, 20, 4)).astype(np.uint8)
    depth = rs.uniform(0, 90, (3, 12, 20)).astype(np.float32)
    depth[0, 0, :4] = [0.0, 0.5, 1.5, 2.5]                                   # rint: half to even
    depth[1, 0, :3] = [65.5351, 65.536, 1e9]                                 # at depth_scale 1000: 65535, saturated, saturated
    render.save_renders(tmp_path / "a", rgba, depth)
    np.testing.assert_array_equal(onboard.load_renders(tmp_path / "a"), rgba)
    for n in range(3):
        got = np.array(Image.open(str(tmp_path / "a" / f"{n:06d}_depth.png")))
        assert got.dtype == np.uint16 or got.max() <= 65535
        np.testing.assert_array_equal(got.astype(np.int64), np.minimum(np.rint(depth[n].astype(np.float64)), 65535).astype(np.int64))
    assert np.array(Image.open(str(tmp_path / "a" / "000000_depth.png")))[0, :4].tolist() == [0, 0, 2, 2]
    render.save_renders(tmp_path / "b", rgba, depth, depth_scale=1000.0)
    got = np.array(Image.open(str(tmp_path / "b" / "000001_depth.png"))).astype(np.int64)
    np.testing.assert_array_equal(got, np.minimum(np.rint(depth[1].astype(np.float64) * 1000.0), 65535).astype(np.int64))
    assert got[0, :3].tolist() == [65535, 65535, 65535]
    render.save_renders(tmp_path / "c", rgba)                                # no depth: only the views
    assert sorted(os.listdir(tmp_path / "c")) == [f"{n:06d}.png" for n in range(3)]
    with pytest.raises(ValueError):
        render.save_renders(tmp_path / "d", rgba[..., :3])
