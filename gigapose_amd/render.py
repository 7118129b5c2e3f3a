"""Templates from a CAD model: a triangle mesh with per-vertex colours + object poses -> the RGBA renders and depth maps the
reference gets from Panda3D (src/custom_megapose/call_panda3d.py:45-95: one white ambient light, so the colour is the unshaded
albedo; alpha = the binary mask * 255; K = TEMPLATE_K at 480 x 640), drawn ON the GPU by a compute rasteriser
(libgigapose_render.so, C-ABI: include/gigapose_render.h) -- an Instinct accelerator has no OpenGL / EGL stack to render with.

Three kernels: gpr_project (vertices -> 1/256-pixel screen coordinates), gpr_raster (a z-buffer of 64-bit keys, depth bits << 32 |
face, merged with an atomic minimum: the image does not depend on the order of the triangles) and gpr_resolve (keys -> RGBA u8
in the format libgigapose_onboard.so reads, + depth).  The arithmetic is written out in the header and restated in numpy in
gigapose_testing/raster_ref.py; tests/test_gpu_render.py holds the kernels to it bit for bit.

  load_ply(path)                        PLY (ascii / binary little endian) -> vertices f32 (V,3), faces int32 (F,3), colours u8 (V,3) | None
  MeshRenderer                          mesh + poses on the device -> {"rgba" (N,H,W,4) u8, "depth" (N,H,W) f32, "clipped" (N,) int32}
  template_object_poses(poses, zoom)    a copy with the translation scaled (render_bop_templates.py:69-70)
  MeshTemplates                         drop-in for model.template_datasets[name], beside onboard.RenderedTemplates
  save_renders(out_dir, rgba, depth)    {view:06d}.png + {view:06d}_depth.png, the reference's layout; onboard.load_renders reads it
What texture.py and shade.py share with this module lives here, once: read_ply (one pass over a PLY file), key_inputs / resolve_out
(the checks of a resolve's key inputs and of its `out`), Renderer (the checks, the buffers, the chunk loop and the clipped-view
error of the three renderers), TemplateSet (the three template datasets) and host.
Textured models (YCB-V, HB) are drawn by texture.py (libgigapose_texture.so), which takes gpr_project's and gpr_raster's output and
resolves it through a mip-mapped texture; models with neither colour nor texture (T-LESS, ITODD) by shade.py (libgigapose_shade.so),
which lights them; this module stays with vertex colours.  Out of scope here: shading other than ambient, near-plane clipping (a triangle with a vertex behind znear is
dropped and counted), anti-aliasing, big-endian PLY, generating the icosphere poses (the caller passes them).  There is no CPU
fallback: the kernels need the GPU, a missing library is an error.
"""
import ctypes
import os

import numpy as np
import pandas as pd
import torch

from . import _lib
from .onboard import TEMPLATE_K, TemplateOnboarder
from .tensor_collection import PandasTensorCollection

MAX_VIEWS_PER_CALL = 65535                          # the grid's second dimension (gigapose_render.h: Limits)
VIS_BYTES_PER_CALL = 1 << 30                        # default chunking: the visibility buffer of one call stays below this
_render = _lib.SideLibrary("libgigapose_render.so", "gpr")
RENDER_LIB_PATH, lib, _call = _render.path, _render.lib, _render.call


def small_triangle_pixels():
    return int(lib().gpr_small_triangle_pixels())


# ------------------------------------------------------------------------------------------------ PLY
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(data, path):
    if not data.startswith(b"ply"):
        raise ValueError(f"load_ply: {path} is not a PLY file")
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if end < 0 or nl < 0:
        raise ValueError(f"load_ply: {path}: truncated file (no end_header)")
    fmt, elements = None, []
    for ln in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"load_ply: {path}: property before any element")
            kinds = w[1:-1]
            if any(k not in _PLY_TYPES for k in kinds if k != "list") or (kinds[0] == "list") != (len(kinds) == 3):
                raise ValueError(f"load_ply: {path}: cannot read property '{ln.strip()}'")
            elements[-1][2].append((w[-1], kinds))
    if fmt == "binary_big_endian":
        raise ValueError(f"load_ply: {path}: binary_big_endian is not supported")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"load_ply: {path}: unknown format {fmt!r}")
    return fmt, elements, nl + 1


def _read_element(fmt, props, count, data, pos, tokens, path, name):
    """One element -> {property: array} (a list property: a list of arrays); returns the new position."""
    has_list = any(k[0] == "list" for _, k in props)
    cols = {p: [] for p, _ in props}
    if fmt == "binary_little_endian" and not has_list:
        dt = np.dtype([(p, "<" + _PLY_TYPES[k[0]]) for p, k in props])
        if pos + dt.itemsize * count > len(data):
            raise ValueError(f"load_ply: {path}: truncated file (element {name})")
        rec = np.frombuffer(data, dt, count, pos)
        return {p: rec[p] for p, _ in props}, pos + dt.itemsize * count
    if fmt == "ascii" and not has_list:
        want = count * len(props)
        try:
            table = np.asarray(tokens[pos:pos + want], dtype=np.float64)
        except ValueError:
            raise ValueError(f"load_ply: {path}: cannot parse element {name}") from None
        if len(table) != want:
            raise ValueError(f"load_ply: {path}: truncated file (element {name})")
        table = table.reshape(count, len(props))
        return {p: table[:, j].astype(_PLY_TYPES[k[0]]) for j, (p, k) in enumerate(props)}, pos + want
    if fmt == "binary_little_endian" and len(props) == 1:     # the usual face element: try (count, n, indices) rows of one size
        ct, it = ("<" + _PLY_TYPES[k] for k in props[0][1][1:])
        if count and pos < len(data):
            n0 = int(np.frombuffer(data, ct, 1, pos)[0])
            dt = np.dtype([("n", ct), ("i", it, (n0,))])
            if pos + dt.itemsize * count <= len(data):
                rec = np.frombuffer(data, dt, count, pos)
                if (rec["n"] == n0).all():
                    return {props[0][0]: rec["i"]}, pos + dt.itemsize * count
    for _ in range(count):                                       # the general case, row by row
        for p, k in props:
            if fmt == "ascii":
                try:
                    if k[0] == "list":
                        n = int(tokens[pos])
                        cols[p].append(np.asarray(tokens[pos + 1:pos + 1 + n], dtype=np.float64).astype(_PLY_TYPES[k[2]]))
                        if len(cols[p][-1]) != n:
                            raise IndexError
                        pos += 1 + n
                    else:
                        cols[p].append(float(tokens[pos]))
                        pos += 1
                except (IndexError, ValueError):
                    raise ValueError(f"load_ply: {path}: truncated file (element {name})") from None
            else:
                try:
                    if k[0] == "list":
                        n = int(np.frombuffer(data, "<" + _PLY_TYPES[k[1]], 1, pos)[0])
                        pos += np.dtype(_PLY_TYPES[k[1]]).itemsize
                        cols[p].append(np.frombuffer(data, "<" + _PLY_TYPES[k[2]], n, pos))
                        pos += n * np.dtype(_PLY_TYPES[k[2]]).itemsize
                    else:
                        cols[p].append(np.frombuffer(data, "<" + _PLY_TYPES[k[0]], 1, pos)[0])
                        pos += np.dtype(_PLY_TYPES[k[0]]).itemsize
                except ValueError:
                    raise ValueError(f"load_ply: {path}: truncated file (element {name})") from None
    out = {}
    for p, k in props:
        out[p] = cols[p] if k[0] == "list" else np.asarray(cols[p], dtype=np.float64).astype(_PLY_TYPES[k[0]])
    return out, pos


def read_ply(path):
    """One pass over the file -> (path as a string, the header's comment lines as written, {element: {property: array, or a list
    of arrays for a list property whose rows differ in length}}).  Reads `ascii` and `binary_little_endian` with numpy alone;
    names and types come from the header.  ValueError: no PLY file, a truncated one, binary_big_endian.  What load_ply,
    shade.load_ply_with_normals and texture.load_textured_ply are built on."""
    path = os.fspath(path)
    with open(path, "rb") as fh:
        data = fh.read()
    fmt, elements, pos = _ply_header(data, path)
    comments = [ln for ln in data[:pos].decode("ascii", "replace").splitlines() if ln.split()[:1] == ["comment"]]
    tokens = None
    if fmt == "ascii":
        tokens, pos = data[pos:].split(), 0
    got = {}
    for name, count, props in elements:
        got[name], pos = _read_element(fmt, props, count, data, pos, tokens, path, name)
    return path, comments, got


def load_ply(path):
    """-> vertices f32 (V,3), faces int32 (F,3), colours u8 (V,3) or None when the file has no red / green / blue.  Properties
    it does not need (normals, alpha, texture_u / texture_v, ...) are skipped; the face list is `vertex_indices` or
    `vertex_index` of any integer types.  ValueError: a face that is not a triangle, an index >= V, and what read_ply rejects."""
    path, _, got = read_ply(path)
    return ply_mesh(path, got)


def ply_mesh(path, got):
    """load_ply's result from read_ply's elements."""
    if "vertex" not in got or not all(k in got["vertex"] for k in "xyz"):
        raise ValueError(f"load_ply: {path}: no vertex element with x, y, z")
    vert = got["vertex"]
    vertices = np.stack([np.asarray(vert[k], np.float32) for k in "xyz"], axis=1) if len(vert["x"]) else np.zeros((0, 3), np.float32)
    colours = None
    if all(k in vert for k in ("red", "green", "blue")):
        chans = [np.asarray(vert[k]) for k in ("red", "green", "blue")]
        if chans[0].dtype.kind == "f":                           # float colours are 0..1
            chans = [np.rint(np.clip(c, 0.0, 1.0) * 255.0) for c in chans]
        colours = np.stack(chans, axis=1).astype(np.uint8).reshape(-1, 3)
    faces = np.zeros((0, 3), np.int32)
    if "face" in got:
        key = next((k for k in ("vertex_indices", "vertex_index") if k in got["face"]), None)
        if key is None:
            raise ValueError(f"load_ply: {path}: the face element has no vertex_indices / vertex_index list")
        rows = got["face"][key]
        if isinstance(rows, list):
            if any(len(r) != 3 for r in rows):
                raise ValueError(f"load_ply: {path}: a face is not a triangle")
            rows = np.asarray(rows).reshape(-1, 3)
        if rows.ndim != 2 or (len(rows) and rows.shape[1] != 3):
            raise ValueError(f"load_ply: {path}: a face is not a triangle")
        rows = rows.astype(np.int64).reshape(-1, 3)
        if len(rows) and (rows.min() < 0 or rows.max() >= len(vertices)):
            raise ValueError(f"load_ply: {path}: a face index is outside [0, {len(vertices)})")
        faces = rows.astype(np.int32)
    return np.ascontiguousarray(vertices), np.ascontiguousarray(faces), colours


# ------------------------------------------------------------------------------------------------ the renderer
def _k9(K):
    k = np.asarray(K, dtype=np.float32).reshape(9)
    if not (k[6] == 0 and k[7] == 0 and k[8] == 1):
        raise ValueError("the last row of K must be 0, 0, 1")
    return (ctypes.c_float * 9)(*k.tolist())


@torch.no_grad()
def project(vertices, poses, K, znear, out=None):
    """gpr_project: vertices f32 (V,3), poses f32 (N,4,4) on the device -> xy int32 (N,V,2) in 1/256 pixel, depth f32 (N,V).
    N <= 65535.  `out` = (xy, depth) are buffers to write into (their first N views are used)."""
    vertices = _lib.on_device(vertices, torch.float32, (None, 3), "project", "vertices")
    poses = _lib.on_device(poses, torch.float32, (None, 4, 4), "project", "poses")
    V, N = vertices.shape[0], poses.shape[0]
    xy, depth = out if out is not None else (torch.empty(N, V, 2, dtype=torch.int32, device=vertices.device),
                                             torch.empty(N, V, dtype=torch.float32, device=vertices.device))
    _call("gpr_project", vertices, V, poses, N, K if isinstance(K, ctypes.Array) else _k9(K), znear, xy, depth, _lib.stream_ptr())
    return xy[:N], depth[:N]


@torch.no_grad()
def raster(xy, vdepth, faces, H, W, out=None, workspace=None):
    """gpr_raster: xy int32 (N,V,2), vdepth f32 (N,V), faces int32 (F,3) -> vis int64 (N,H,W) holding the unsigned 64-bit keys
    (depth bits << 32 | face; -1 = uncovered), clipped int32 (N,).  `out` = (vis, clipped) and `workspace` (int64, at least
    gpr_raster_workspace_bytes(N, F) bytes) are buffers to use."""
    xy = _lib.on_device(xy, torch.int32, (None, None, 2), "raster", "xy")
    N, V = xy.shape[:2]
    vdepth = _lib.on_device(vdepth, torch.float32, (N, V), "raster", "vdepth")
    faces = _lib.on_device(faces, torch.int32, (None, 3), "raster", "faces")
    F, dev = faces.shape[0], xy.device
    vis, clipped = out if out is not None else (torch.empty(N, H, W, dtype=torch.int64, device=dev),
                                                torch.empty(N, dtype=torch.int32, device=dev))
    need = _render.value("gpr_raster_workspace_bytes", N, F)
    if workspace is None:
        workspace = torch.empty(-(-need // 8), dtype=torch.int64, device=dev)
    if workspace.numel() * workspace.element_size() < need or vis.numel() < N * H * W or clipped.numel() < N:
        raise ValueError("raster: a buffer is too small")
    _call("gpr_raster", xy, vdepth, V, faces, F, N, H, W, vis, clipped, workspace, _lib.stream_ptr())
    return vis[:N], clipped[:N]


def key_inputs(who, vis, xy, vdepth, faces):
    """What every resolve takes beside its colour inputs, checked: -> vis int64 (N,H,W), xy int32 (N,V,2), vdepth f32 (N,V), faces
    int32 (F,3) and N, H, W, V, F."""
    vis = _lib.on_device(vis, torch.int64, (None, None, None), who, "vis")
    N, H, W = vis.shape
    xy = _lib.on_device(xy, torch.int32, (N, None, 2), who, "xy")
    V = xy.shape[1]
    vdepth = _lib.on_device(vdepth, torch.float32, (N, V), who, "vdepth")
    faces = _lib.on_device(faces, torch.int32, (None, 3), who, "faces")
    return vis, xy, vdepth, faces, N, H, W, V, faces.shape[0]


def resolve_out(who, out, N, H, W, device, unlit=False):
    """`out` of a resolve, or new buffers: rgba u8 (N,H,W,4), depth f32 (N,H,W) [, unlit int32 (N,)], checked."""
    if out is None:
        out = (torch.empty(N, H, W, 4, dtype=torch.uint8, device=device), torch.empty(N, H, W, dtype=torch.float32, device=device))
        out += (torch.empty(N, dtype=torch.int32, device=device),) if unlit else ()
    if [tuple(t.shape) for t in out] != [(N, H, W, 4), (N, H, W)] + [(N,)] * unlit:
        raise ValueError(f"{who}: out must be rgba (N,H,W,4)" + (", depth (N,H,W) and unlit (N,)" if unlit else " and depth (N,H,W)"))
    return out


@torch.no_grad()
def resolve(vis, xy, vdepth, faces, colours, out=None):
    """gpr_resolve: the keys -> rgba u8 (N,H,W,4), depth f32 (N,H,W); `out` = (rgba, depth) are buffers to write into."""
    vis, xy, vdepth, faces, N, H, W, V, F = key_inputs("resolve", vis, xy, vdepth, faces)
    colours = _lib.on_device(colours, torch.uint8, (V, 3), "resolve", "colours")
    rgba, depth = resolve_out("resolve", out, N, H, W, vis.device)
    _call("gpr_resolve", vis, xy, vdepth, V, faces, F, colours, N, H, W, rgba, depth, _lib.stream_ptr())
    return rgba, depth


class KeyBuffers:
    """What drawing up to n views of a mesh of V vertices and F faces at H x W needs, allocated once and used chunk after chunk:
    xy, vdepth, the keys `vis` and gpr_raster's workspace.  .draw(vertices, faces, poses32 (nb <= n, 4, 4), K9, znear, clipped
    int32 (nb,), written) is project -> raster and returns (keys (nb,H,W), xy, vdepth), views of the buffers."""

    def __init__(self, n, V, F, H, W, device):
        self.H, self.W = H, W
        self.xy = torch.empty(n, V, 2, dtype=torch.int32, device=device)
        self.vdepth = torch.empty(n, V, dtype=torch.float32, device=device)
        self.vis = torch.empty(n, H, W, dtype=torch.int64, device=device)
        self.work = torch.empty(max(1, -(-_render.value("gpr_raster_workspace_bytes", n, F) // 8)), dtype=torch.int64, device=device)

    def draw(self, vertices, faces, poses32, K9, znear, clipped):
        pxy, pz = project(vertices, poses32, K9, znear, out=(self.xy, self.vdepth))
        keys, _ = raster(pxy, pz, faces, self.H, self.W, out=(self.vis, clipped), workspace=self.work)
        return keys, pxy, pz


def views_step(views_per_call, H, W):
    """The chunk size of the renderers: by default the keys of one call stay below VIS_BYTES_PER_CALL."""
    if views_per_call is None:
        views_per_call = max(1, VIS_BYTES_PER_CALL // (H * W * 8))
    return max(1, min(int(views_per_call), MAX_VIEWS_PER_CALL))


def raise_clipped(who, clipped, F, znear):
    """The renderers' error for the first view that drops a triangle; one host synchronisation."""
    bad = torch.nonzero(clipped).flatten().tolist()
    if bad:
        raise ValueError(f"{who}: view {bad[0]} drops {int(clipped[bad[0]])} of {F} triangles: a vertex lies behind znear = {znear}, "
                         f"beyond 16384 px or is not finite (views {bad[:8]}{' ...' if len(bad) > 8 else ''}; there is no "
                         "near-plane clipping -- on_clipped='ignore' renders what is left)")


def template_object_poses(obj_poses, zoom=0.4):
    """A copy of the (N,4,4) object poses with the translation scaled: `template_poses[:, :3, 3] *= 0.4  # zoom to object`
    (src/scripts/render_bop_templates.py:69-70).  The poses themselves (obj_poses_level1.npy, 162 views) come from the caller."""
    if isinstance(obj_poses, torch.Tensor):
        out = obj_poses.clone()
    else:
        out = np.array(obj_poses, copy=True)
    out[..., :3, 3] = out[..., :3, 3] * zoom
    return out


class Renderer:
    """What MeshRenderer, texture.TexturedMeshRenderer and shade.ShadedMeshRenderer share: the frame, the camera, znear, the checks
    of the mesh and the poses, the result's buffers, the chunk loop over render.KeyBuffers and the clipped-view error.  A
    subclass names itself in `who`, passes its own inputs through ._draw and supplies
      ._prepare(vertices, faces, poses, **inputs) -> state    its inputs checked (colours / UVs and pyramid / normals and tables)
      ._resolve_chunk(state, keys, xy, vdepth, a, b, out)     views a..b of the result `out` from the keys of one chunk
    and, in `counters`, the names of the int32 (N,) counts its resolve writes beside "clipped"."""
    who = None
    no_colour = None                                # the wording of `colours=None` without `colour`
    counters = ()

    def __init__(self, H=480, W=640, K=TEMPLATE_K, znear=1e-3):
        self.H, self.W, self.znear = int(H), int(W), float(znear)
        self._K = _k9(K)

    def _colours(self, V, colours, colour, device):
        if colours is None:
            if colour is None:
                raise ValueError(f"{self.who}: {self.no_colour}")
            colours = torch.tensor([colour], dtype=torch.uint8, device=device).expand(V, 3)
        return _lib.on_device(colours, torch.uint8, (V, 3), self.who, "colours")

    @torch.no_grad()
    def _draw(self, vertices, faces, poses, views_per_call, on_clipped, **inputs):
        """-> {"rgba", "depth", "clipped"} + one entry per name in `counters`."""
        who = self.who
        if on_clipped not in ("raise", "ignore"):
            raise ValueError(f"{who}: on_clipped must be 'raise' or 'ignore'")
        vertices = _lib.on_device(vertices, torch.float32, (None, 3), who, "vertices")
        faces = _lib.on_device(faces, torch.int32, (None, 3), who, "faces")
        poses = _lib.on_device(poses, torch.float32, (None, 4, 4), who, "poses")
        V, F, N = vertices.shape[0], faces.shape[0], poses.shape[0]
        dev = vertices.device
        state = self._prepare(vertices, faces, poses, **inputs)
        H, W = self.H, self.W
        step = views_step(views_per_call, H, W)
        out = {"rgba": torch.empty(N, H, W, 4, dtype=torch.uint8, device=dev), "depth": torch.empty(N, H, W, dtype=torch.float32, device=dev)}
        out.update({k: torch.empty(N, dtype=torch.int32, device=dev) for k in ("clipped",) + tuple(self.counters)})
        buffers = KeyBuffers(min(N, step), V, F, H, W, dev)
        for _, a, b in _lib.chunked(N, step):
            keys, pxy, pz = buffers.draw(vertices, faces, poses[a:b], self._K, self.znear, out["clipped"][a:b])
            self._resolve_chunk(state, keys, pxy, pz, a, b, out)
        if on_clipped == "raise":
            raise_clipped(who, out["clipped"], F, self.znear)
        return out


class MeshRenderer(Renderer):
    """vertices f32 (V,3), faces int32 (F,3), colours u8 (V,3), poses f32 (N,4,4), all on the device -> rgba u8 (N,H,W,4) in the
    format gpo_alpha_boxes / gpo_crop_templates read, depth f32 (N,H,W) in model units (0 where nothing is drawn), clipped
    int32 (N,).  Poses are object -> camera in the OpenCV convention (x right, y down, z forward), what the reference's load_pose
    returns; pixel centres sit at integer coordinates.  znear is in model units."""
    who = "MeshRenderer"
    no_colour = "the mesh has no vertex colours and textures are out of scope: pass colour=(r, g, b)"

    def __call__(self, vertices, faces, colours, poses, views_per_call=None, colour=None, on_clipped="raise"):
        """`colours=None` needs `colour=(r, g, b)`, painted on every vertex (the reference paints T-LESS a uniform grey,
        src/lib3d/pyrender.py:90-95).  A view with a dropped triangle (a vertex behind znear, beyond 16384 px or not finite, or a
        face index outside the mesh) raises ValueError naming it unless on_clipped="ignore".  One host synchronisation: the
        read of the clipped counts."""
        return self._draw(vertices, faces, poses, views_per_call, on_clipped, colours=colours, colour=colour)

    def _prepare(self, vertices, faces, poses, colours, colour):
        return faces, self._colours(vertices.shape[0], colours, colour, vertices.device)

    def _resolve_chunk(self, state, keys, pxy, pz, a, b, out):
        resolve(keys, pxy, pz, *state, out=(out["rgba"][a:b], out["depth"][a:b]))


def host(a, dtype=None):
    """A tensor or anything numpy reads -> a host array; with `dtype`, a C-contiguous COPY of that type (PIL hands out read-only
    arrays, and torch.from_numpy wants a writable one)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else np.array(a, dtype=dtype, order="C")


def _host_mesh(mesh, who):
    if isinstance(mesh, (str, os.PathLike)):
        mesh = load_ply(mesh)
    if isinstance(mesh, dict):
        mesh = (mesh["vertices"], mesh["faces"], mesh.get("colours"))
    v, f, c = mesh
    v, f = torch.from_numpy(host(v, np.float32)), torch.from_numpy(host(f, np.int32))
    c = None if c is None else torch.from_numpy(host(c, np.uint8))
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or (c is not None and tuple(c.shape) != tuple(v.shape)):
        raise ValueError(f"{who}: expected vertices (V,3), faces (F,3), colours (V,3) or None")
    if len(f) and (int(f.min()) < 0 or int(f.max()) >= len(v)):
        raise ValueError(f"{who}: a face index is outside [0, {len(v)})")
    return v, f, c


class TemplateSet:
    """What MeshTemplates, texture.TexturedMeshTemplates and shade.ShadedMeshTemplates share: a drop-in for
    `model.template_datasets[name]` whose item i is a PandasTensorCollection with .rgb (N,3,T,T) .mask (N,T,T) .K (3,3) .M (N,3,3)
    .poses (N,4,4) on the device.  The objects stay on the HOST; every __getitem__ uploads one, renders its N views on the device
    and hands the device renders to TemplateOnboarder: no render crosses PCIe.  A subclass names itself in `who` and supplies
    ._host_object(o, obj) -> (host tensors of the mesh | None, poses) and ._render_object(mesh on the device, poses)."""
    who = None

    def __init__(self, objects, renderer, K, device, target_size):
        """renderer: K (3,3) f32 -> the subclass's renderer."""
        self.device = torch.device(device)
        K = np.asarray(TEMPLATE_K if K is None else K, dtype=np.float32).reshape(3, 3)
        self.K = torch.as_tensor(K)
        self.renderer = renderer(K)
        self.onboard = TemplateOnboarder(target_size)
        self._meshes, self._poses = [], []
        for o, obj in enumerate(objects):
            mesh, poses = self._host_object(o, obj)
            p = torch.from_numpy(host(poses, np.float32))
            if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
                raise ValueError(f"{self.who}: object {o}: expected poses (N, 4, 4), got {tuple(p.shape)}")
            self._meshes.append(mesh)
            self._poses.append(p)

    def __len__(self):
        return len(self._meshes)

    @torch.no_grad()
    def render(self, i):
        """The device renders of object i: the renderer's result."""
        if self.device.type != "cuda":
            raise _lib.GigaPoseHipError(f"{self.who} needs a GPU device (no CPU fallback)")
        mesh = tuple(None if t is None else t.to(self.device) for t in self._meshes[i])
        try:
            return self._render_object(mesh, self._poses[i].to(self.device))
        except ValueError as e:
            raise ValueError(f"{self.who}: object {i}: {e}") from None

    @torch.no_grad()
    def __getitem__(self, i):
        rgba = self.render(i)["rgba"]
        try:
            out = self.onboard(rgba)
        except ValueError as e:
            raise ValueError(f"{self.who}: object {i}: {e}") from None
        return PandasTensorCollection(infos=pd.DataFrame(), K=self.K.to(self.device), rgb=out["rgb"], mask=out["mask"], M=out["M"],
                                      poses=self._poses[i].to(self.device))


class MeshTemplates(TemplateSet):
    """Drop-in for `model.template_datasets[name]`, beside onboard.RenderedTemplates: item i is a PandasTensorCollection with
    .rgb (N,3,T,T) .mask (N,T,T) .K (3,3) .M (N,3,3) .poses (N,4,4) on the device.

    objects: list of (mesh, poses) -- mesh a PLY path, a (vertices, faces, colours) tuple or a dict with those keys; poses
    (N,4,4) object -> camera as the reference's load_pose returns them (template_object_poses applies the reference's zoom), in
    bank order.  `colour=(r, g, b)` paints meshes without vertex colours.  The meshes stay on the HOST; every __getitem__ uploads
    the mesh, renders its N views on the device and hands the device renders to TemplateOnboarder: no render crosses PCIe."""
    who = "MeshTemplates"

    def __init__(self, objects, K=None, device="cuda", target_size=224, H=480, W=640, znear=1e-3, colour=None):
        self.colour = colour
        super().__init__(objects, lambda K: MeshRenderer(H, W, K, znear), K, device, target_size)

    def _host_object(self, o, obj):
        mesh, poses = obj
        m = _host_mesh(mesh, f"{self.who}: object {o}")
        if m[2] is None and self.colour is None:
            raise ValueError(f"{self.who}: object {o} has no vertex colours and textures are out of scope: pass colour=(r, g, b)")
        return m, poses

    def _render_object(self, mesh, poses):
        return self.renderer(*mesh, poses, colour=self.colour)


def save_renders(out_dir, rgba, depth=None, depth_scale=1.0):
    """The reference's layout (call_panda3d.py:84-95): `{view:06d}.png` as RGBA and `{view:06d}_depth.png` as 16-bit grey holding
    rint(depth * depth_scale), saturated at 65535 -- the reference stores millimetres, so a model in metres takes
    depth_scale=1000.  onboard.load_renders(out_dir) returns the same rgba."""
    from PIL import Image

    rgba = host(rgba)
    if not (rgba.dtype == np.uint8 and rgba.ndim == 4 and rgba.shape[3] == 4):
        raise ValueError(f"save_renders: expected u8 renders (N, H, W, 4), got {rgba.dtype} {rgba.shape}")
    if depth is not None:
        depth = host(depth)
        if depth.shape != rgba.shape[:3]:
            raise ValueError(f"save_renders: depth {depth.shape} does not match the renders {rgba.shape[:3]}")
    out_dir = os.fspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    for n in range(len(rgba)):
        Image.fromarray(rgba[n], "RGBA").save(os.path.join(out_dir, f"{n:06d}.png"))
        if depth is not None:
            d = np.clip(np.rint(depth[n].astype(np.float64) * depth_scale), 0, 65535).astype(np.uint16)
            Image.fromarray(d).save(os.path.join(out_dir, f"{n:06d}_depth.png"))
