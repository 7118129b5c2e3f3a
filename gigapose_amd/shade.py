"""Templates from an UNTEXTURED, UNCOLOURED CAD model (T-LESS, ITODD): mesh + object poses -> LIT RGBA renders and depth maps,
drawn ON the GPU.  render.py draws "one white ambient light": such a model becomes a silhouette of one RGB value, and the patch
features inside the mask carry no geometry.  The reference renders these two datasets with BlenderProc instead
(src/scripts/render_bop_templates.py:124 -> src/lib3d/blenderproc.py: eight point lights around the camera, a uniform grey of
0.4), so that the lighting creates the template's interior signal.  render.py's gpr_project and gpr_raster give the visibility
keys; libgigapose_shade.so (C-ABI: include/gigapose_shade.h) computes area-weighted vertex normals as integer sums
(gpl_vertex_normals) and turns the keys into diffusely shaded colours (gpl_shade: Lambert's cosine, inverse-square fall-off,
point lights in camera coordinates, two host tables for the transfer curves).  The arithmetic is written out in the header and
restated in numpy in gigapose_testing/shade_ref.py; tests/test_gpu_shade.py holds the kernels to it bit for bit.

  vertex_normals(vertices, faces)       smooth normals f64 (V,3) on the device; raises on a face beyond the range guard
  srgb_tables(T) / linear_tables(T)     (decode f64 (256,), encode u8 (T,)): the transfer curves, computed on the host
  blenderproc_lights(units_per_metre)   the reference's eight lights as (8,4) f64: x, y, z in our camera convention, intensity
  load_ply_with_normals(path)           render.load_ply's result + nx, ny, nz as f64 (V,3) | None
  shade(...)                            thin wrapper of gpl_shade
  ShadedMeshRenderer                    mesh + poses on the device -> {"rgba", "depth", "clipped", "unlit"}
  ShadedMeshTemplates                   drop-in for model.template_datasets[name], beside render.MeshTemplates
WHAT THIS IS NOT: a reproduction of Blender's image.  The model is diffuse only; the Principled shader's specular lobe, the
100-sample path tracing (no shadows, no inter-reflection here) and Blender's view transform are not modelled, and nobody has
compared the output with a Cycles render.  The contract is the header.  Also out of scope, as in render.py: near-plane clipping,
anti-aliasing.  There is no CPU fallback.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib, render
from .onboard import TEMPLATE_K

RANGE, NO_NORMAL = 1, 2                             # gigapose_shade.h: GPL_RANGE, GPL_NO_NORMAL
SMOOTH, FLAT = 0, 1                                 # gigapose_shade.h: GPL_SMOOTH, GPL_FLAT
MAX_LIGHTS = 16                                     # gigapose_shade.h: GPL_MAX_LIGHTS
TLESS_GREY = (102, 102, 102)                        # 0.4 x 255: the reference's T-LESS grey (blenderproc.py:48)
_MODES = {"smooth": SMOOTH, "flat": FLAT, SMOOTH: SMOOTH, FLAT: FLAT}
_shade = _lib.SideLibrary("libgigapose_shade.so", "gpl")
SHADE_LIB_PATH, lib, _call = _shade.path, _shade.lib, _shade.call


# ------------------------------------------------------------------------------------------------ normals
def normal_unit(vertices):
    """The power of two gpl_vertex_normals multiplies a cross product with, from the mesh's bounding box: with E the largest
    extent, E < 2^e, a component u_i*v_j - u_j*v_i of any face's cross product stays below 2 E^2 < 2^(2e+1), so unit = 2^(39-2e)
    keeps every quantised component below the guard of 2^40 -- no face of a mesh with finite vertices can reach it.  (A mesh
    of one point, or one that is not finite, gets 1.0: the flags report the latter.)  vertices: a tensor or an array."""
    v = vertices.detach() if isinstance(vertices, torch.Tensor) else torch.from_numpy(np.asarray(vertices, np.float32))
    if v.numel() == 0:
        return 1.0
    extent = float((v.double().amax(dim=0) - v.double().amin(dim=0)).max())
    if not (extent > 0.0 and math.isfinite(extent)):
        return 1.0
    e = math.frexp(extent)[1]                       # extent = m * 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, max(-1000, min(1000, 39 - 2 * e)))


@torch.no_grad()
def vertex_normals_raw(vertices, faces, unit, out=None):
    """gpl_vertex_normals: vertices f32 (V,3), faces int32 (F,3) on the device -> acc int64 (V,3), flags int32 (V,), normals f64
    (V,3); `out` = (acc, flags, normals) are buffers to write into (the call initialises them)."""
    who = "vertex_normals"
    vertices = _lib.on_device(vertices, torch.float32, (None, 3), who, "vertices")
    faces = _lib.on_device(faces, torch.int32, (None, 3), who, "faces")
    V, dev = vertices.shape[0], vertices.device
    acc, flags, normals = out if out is not None else (torch.empty(V, 3, dtype=torch.int64, device=dev),
                                                       torch.empty(V, dtype=torch.int32, device=dev),
                                                       torch.empty(V, 3, dtype=torch.float64, device=dev))
    if tuple(acc.shape) != (V, 3) or tuple(flags.shape) != (V,) or tuple(normals.shape) != (V, 3):
        raise ValueError(f"{who}: out must be acc (V,3), flags (V,) and normals (V,3)")
    _call("gpl_vertex_normals", vertices, V, faces, faces.shape[0], unit, acc, flags, normals, _lib.stream_ptr())
    return acc, flags, normals


@torch.no_grad()
def vertex_normals(vertices, faces):
    """Smooth, area-weighted vertex normals f64 (V,3) on the device; a vertex no face uses, or whose faces cancel, gets 0, 0, 0
    (gpl_shade counts the pixels it leaves without a normal in "unlit").  The unit comes from normal_unit.  ValueError, naming
    the vertex: a face with a cross product beyond the range guard, which takes a vertex that is not finite.  Two host
    synchronisations: the bounding box and the flags."""
    _, flags, normals = vertex_normals_raw(vertices, faces, normal_unit(vertices))
    bad = torch.nonzero(flags & RANGE).flatten()
    if len(bad):
        v = int(bad[0])
        raise ValueError(f"vertex_normals: vertex {v} = {vertices[v].tolist()} belongs to a face whose cross product is not finite or "
                         f"leaves the range of the integer sum ({len(bad)} such vertices)")
    return normals


# ------------------------------------------------------------------------------------------------ tables and lights
def srgb_tables(T=4096):
    """(decode, encode) of the sRGB transfer function, computed in float64 on the host: decode f64 (256,) maps a colour byte c to
    the linear value of c / 255; encode u8 (T,) maps the linear value i / (T-1) to the byte rint(255 * srgb(i / (T-1))).
    Resolution: the kernel rounds a linear value to the nearest of T levels, an error of at most 1 / (2 (T-1)); the curve's
    steepest slope is 12.92 (its linear toe), so the encoded value is off by at most 12.92 * 255 / (2 (T-1)) code values before
    its own rounding -- at T = 4096, 12.92 * 255 / 4095 = 0.80 per level, 0.40 < 1/2 from rounding: one level never skips a
    code value, and a colour at irradiance 1 comes back as itself (tests/test_shade_host.py)."""
    T = int(T)
    if not 256 <= T <= 65536:
        raise ValueError(f"srgb_tables: 256 <= T <= 65536, got {T}")
    c = np.arange(256, dtype=np.float64) / 255.0
    decode = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    x = np.arange(T, dtype=np.float64) / (T - 1)
    s = np.where(x <= 0.0031308, x * 12.92, 1.055 * x ** (1.0 / 2.4) - 0.055)
    return decode, np.clip(np.rint(s * 255.0), 0, 255).astype(np.uint8)


def linear_tables(T=256):
    """The identity pair: decode[c] = c / 255, encode[i] = rint(255 i / (T-1)).  With T = 256, no light and ambient = 1 the
    shaded render IS gpr_resolve's (c / 255 * 255 + 1/2 floors to c for every byte)."""
    T = int(T)
    if not 256 <= T <= 65536:
        raise ValueError(f"linear_tables: 256 <= T <= 65536, got {T}")
    return np.arange(256, dtype=np.float64) / 255.0, np.rint(np.arange(T, dtype=np.float64) * 255.0 / (T - 1)).astype(np.uint8)


def blenderproc_lights(units_per_metre, watts=50.0):
    """The eight point lights of the reference (src/lib3d/blenderproc.py:27-37: x, y in {-1, 1}, z in {0, 1} metres about a camera
    at the origin, 50 W each) as (8,4) f64 rows x, y, z, intensity in OUR camera convention and model units: Blender's camera
    looks down -z with y up, so Blender's (x, y, z) is OpenCV's (x, -y, -z), times units_per_metre (1000 for BOP's millimetre
    models).  Four lights sit in the camera's plane, four one metre behind it.  Intensity: Blender's point light of P watts
    lights a diffuse surface like a radiant intensity of P / (4 pi^2) per steradian; distances are in model units, hence
    * units_per_metre^2.  NOT VALIDATED: nobody has compared this with a Cycles render.  The Principled shader's specular lobe,
    the 100-sample path tracing and Blender's view transform are not modelled; the contract is include/gigapose_shade.h."""
    upm = float(units_per_metre)
    rows = [(x * upm, -y * upm, -z * upm, float(watts) / (4.0 * math.pi ** 2) * upm * upm) for x in (-1, 1) for y in (-1, 1) for z in (0, 1)]
    return np.asarray(rows, np.float64)


def load_ply_with_normals(path):
    """-> vertices, faces, colours as render.load_ply returns them, + normals f64 (V,3) from the vertex properties nx, ny, nz, or
    None when the file has none (BOP's model files usually carry them; load_ply skips them)."""
    path, _, got = render.read_ply(path)
    vert, normals = got.get("vertex", {}), None
    if all(k in vert for k in ("nx", "ny", "nz")):
        normals = np.ascontiguousarray(np.stack([np.asarray(vert[k], np.float64) for k in ("nx", "ny", "nz")], axis=1).reshape(-1, 3))
    return render.ply_mesh(path, got) + (normals,)


def _tables(tables, who):
    decode, encode = tables
    decode = np.ascontiguousarray(np.asarray(decode.cpu() if isinstance(decode, torch.Tensor) else decode, dtype=np.float64))
    encode = np.asarray(encode.cpu() if isinstance(encode, torch.Tensor) else encode)
    if decode.shape != (256,) or encode.ndim != 1 or not 256 <= len(encode) <= 65536 or encode.dtype != np.uint8:
        raise ValueError(f"{who}: tables must be (decode f64 (256,), encode u8 (T,)) with 256 <= T <= 65536")
    return torch.from_numpy(decode), torch.from_numpy(np.ascontiguousarray(encode))


def _lights(lights, who):
    rows = np.ascontiguousarray(np.asarray(lights, dtype=np.float64).reshape(-1, 4)) if lights is not None and len(lights) else np.zeros((0, 4))
    if len(rows) > MAX_LIGHTS:
        raise ValueError(f"{who}: at most {MAX_LIGHTS} lights, got {len(rows)}")
    return rows


# ------------------------------------------------------------------------------------------------ the entry point
@torch.no_grad()
def shade(vis, xy, vdepth, faces, colours, vertices, normals, poses, K, lights, ambient, decode, encode, mode, out=None):
    """gpl_shade: the keys of render.raster + colours u8 (V,3) + vertices f32 (V,3) (flat) or normals f64 (V,3) (smooth) + poses f32
    (N,4,4), all on the device; K 3x3; lights (L,4) f64 on the HOST; decode f64 (256,), encode u8 (T,) on the device -> rgba u8
    (N,H,W,4), depth f32 (N,H,W), unlit int32 (N,); `out` = (rgba, depth, unlit) are buffers to write into."""
    who = "shade"
    if mode not in _MODES:
        raise ValueError(f"{who}: mode must be 'smooth' or 'flat'")
    mode = _MODES[mode]
    vis, xy, vdepth, faces, N, H, W, V, F = render.key_inputs(who, vis, xy, vdepth, faces)
    colours = _lib.on_device(colours, torch.uint8, (V, 3), who, "colours")
    if mode == FLAT:
        vertices, normals = _lib.on_device(vertices, torch.float32, (V, 3), who, "vertices"), None
    else:
        vertices, normals = None, _lib.on_device(normals, torch.float64, (V, 3), who, "normals")
    poses = _lib.on_device(poses, torch.float32, (N, 4, 4), who, "poses")
    decode = _lib.on_device(decode, torch.float64, (256,), who, "decode")
    encode = _lib.on_device(encode, torch.uint8, (None,), who, "encode")
    rows = _lights(lights, who)
    rgba, depth, unlit = render.resolve_out(who, out, N, H, W, vis.device, unlit=True)
    host_lights = (ctypes.c_double * max(1, rows.size))(*rows.reshape(-1).tolist())
    _call("gpl_shade", vis, xy, vdepth, V, faces, F, colours, vertices, normals, poses, K if isinstance(K, ctypes.Array) else render._k9(K), host_lights,
          len(rows), ambient, decode, encode, encode.shape[0], mode, N, H, W, rgba, depth, unlit, _lib.stream_ptr())
    return rgba, depth, unlit


# ------------------------------------------------------------------------------------------------ the renderer
class ShadedMeshRenderer(render.Renderer):
    """vertices f32 (V,3), faces int32 (F,3), colours u8 (V,3), poses f32 (N,4,4), all on the device -> rgba u8 (N,H,W,4), depth f32
    (N,H,W), clipped int32 (N,) as render.MeshRenderer returns them (same poses, K, pixel centres, znear), + unlit int32 (N,):
    the covered pixels of a view that had no usable normal and show the ambient term alone.
    lights: (L,4) rows x, y, z, intensity in CAMERA coordinates (OpenCV) and model units, L <= 16; ambient: irradiance added
    everywhere; tables: (decode, encode) as srgb_tables / linear_tables return them; mode: "smooth" (vertex normals, interpolated
    perspective-correctly) or "flat" (the face's own normal)."""
    who = "ShadedMeshRenderer"
    no_colour = "the mesh has no vertex colours: pass colour=(r, g, b)"
    counters = ("unlit",)

    def __init__(self, H=480, W=640, K=TEMPLATE_K, znear=1e-3, lights=None, ambient=0.0, tables=None, mode="smooth"):
        super().__init__(H, W, K, znear)
        if mode not in _MODES:
            raise ValueError(f"{self.who}: mode must be 'smooth' or 'flat'")
        self.mode = _MODES[mode]
        self.lights, self.ambient = _lights(lights, self.who), float(ambient)
        self._decode, self._encode = _tables(srgb_tables() if tables is None else tables, self.who)
        self._device_tables = {}

    def _on(self, dev):
        if dev not in self._device_tables:
            self._device_tables[dev] = (self._decode.to(dev), self._encode.to(dev))
        return self._device_tables[dev]

    def __call__(self, vertices, faces, colours, poses, normals=None, views_per_call=None, colour=None, on_clipped="raise"):
        """`colours=None` needs `colour=(r, g, b)`, painted on every vertex.  `normals` f64 (V,3) on the device (from the model
        file) are used in smooth mode; None computes them with vertex_normals.  Chunking, the clipped-view error and its host
        synchronisation are MeshRenderer's."""
        return self._draw(vertices, faces, poses, views_per_call, on_clipped, colours=colours, colour=colour, normals=normals)

    def _prepare(self, vertices, faces, poses, colours, colour, normals):
        V, dev = vertices.shape[0], vertices.device
        colours = self._colours(V, colours, colour, dev)
        if self.mode == SMOOTH:
            normals = vertex_normals(vertices, faces) if normals is None else _lib.on_device(normals, torch.float64, (V, 3), self.who, "normals")
        return faces, colours, vertices, normals, poses, self._on(dev)

    def _resolve_chunk(self, state, keys, pxy, pz, a, b, out):
        faces, colours, vertices, normals, poses, tables = state
        shade(keys, pxy, pz, faces, colours, vertices, normals, poses[a:b], self._K, self.lights, self.ambient, *tables, self.mode,
              out=(out["rgba"][a:b], out["depth"][a:b], out["unlit"][a:b]))


def _host_mesh(mesh, who):
    """-> vertices, faces, colours | None, normals | None as host tensors."""
    if isinstance(mesh, (str, os.PathLike)):
        mesh = load_ply_with_normals(mesh)
    if isinstance(mesh, dict):
        mesh = (mesh["vertices"], mesh["faces"], mesh.get("colours"), mesh.get("normals"))
    if len(mesh) == 3:
        mesh = tuple(mesh) + (None,)
    v, f, c = render._host_mesh(mesh[:3], who)
    n = mesh[3]
    if n is not None:
        n = torch.from_numpy(render.host(n, np.float64))
        if tuple(n.shape) != tuple(v.shape):
            raise ValueError(f"{who}: expected normals (V,3), got {tuple(n.shape)}")
    return v, f, c, n


class ShadedMeshTemplates(render.TemplateSet):
    """Drop-in for `model.template_datasets[name]`, beside render.MeshTemplates: item i is the same PandasTensorCollection, .rgb
    (N,3,T,T) .mask (N,T,T) .K (3,3) .M (N,3,3) .poses (N,4,4) on the device.

    objects: list of (mesh, poses) -- mesh a PLY path, a (vertices, faces, colours[, normals]) tuple or a dict with those keys;
    poses (N,4,4) as for MeshTemplates.  colour paints meshes without vertex colours: the default is the reference's T-LESS grey.
    lights: (L,4) rows in camera coordinates and model units; None takes blenderproc_lights(units_per_metre) (BOP models are in
    millimetres).  normals: "file" -- the model file's nx, ny, nz (an error if it has none), "smooth" -- computed by
    gpl_vertex_normals, "flat" -- every face its own normal.  The meshes stay on the HOST; every __getitem__ uploads the mesh,
    renders and lights its N views on the device and hands the device renders to TemplateOnboarder: no render crosses PCIe.
    What the lighting model leaves out of Blender's render is listed in the module's docstring; no effect on pose accuracy has
    been measured."""

    who = "ShadedMeshTemplates"

    def __init__(self, objects, K=None, device="cuda", target_size=224, H=480, W=640, znear=1e-3, colour=TLESS_GREY, lights=None,
                 ambient=0.0, tables=None, normals="smooth", units_per_metre=1000.0):
        if normals not in ("file", "smooth", "flat"):
            raise ValueError("ShadedMeshTemplates: normals must be 'file', 'smooth' or 'flat'")
        self.colour, self.normals = colour, normals
        if lights is None:
            lights = blenderproc_lights(units_per_metre)
        super().__init__(objects, lambda K: ShadedMeshRenderer(H, W, K, znear, lights, ambient, tables, "flat" if normals == "flat" else "smooth"),
                         K, device, target_size)

    def _host_object(self, o, obj):
        mesh, poses = obj
        m = _host_mesh(mesh, f"{self.who}: object {o}")
        if m[2] is None and self.colour is None:
            raise ValueError(f"{self.who}: object {o} has no vertex colours: pass colour=(r, g, b)")
        if self.normals == "file" and m[3] is None:
            raise ValueError(f"{self.who}: object {o} carries no normals (nx, ny, nz): use normals='smooth' or 'flat'")
        return m, poses

    def _render_object(self, mesh, poses):
        v, f, c, n = mesh
        return self.renderer(v, f, c, poses, normals=n if self.normals == "file" else None, colour=self.colour)
