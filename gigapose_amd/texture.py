"""Templates from a TEXTURED CAD model (YCB-V, HB: PLY files with texture_u / texture_v per vertex and `comment TextureFile
obj_0000NN.png`, no usable vertex colours): mesh + per-corner UVs + one texture image + object poses -> the RGBA renders and depth
maps the reference gets from Panda3D with mip-mapped texture filtering (src/megapose/panda3d_renderer/
panda3d_scene_renderer.py:70-71), drawn ON the GPU.  render.py's gpr_project and gpr_raster give the visibility keys;
libgigapose_texture.so (C-ABI: include/gigapose_texture.h) builds the mip pyramid (gpt_build_mips) and turns the keys into
colours with perspective-correct UVs, an analytic level of detail and trilinear, repeat-wrapped sampling (gpt_resolve).  The
arithmetic is written out in the header and restated in numpy in gigapose_testing/texture_ref.py; tests/test_gpu_texture.py
holds the kernels to it bit for bit.

  load_textured_ply(path)     PLY -> {"vertices", "faces", "colours" | None, "corner_uv" f32 (F,3,2), "texture_file" | None}
  load_texture(path)          any PIL-readable image -> rgb u8 (Ht,Wt,3)
  corner_uv_from_vertices     per-vertex UVs (V,2) + faces -> per-corner UVs (F,3,2)
  build_mips / resolve_textured  thin wrappers of the two entry points
  TexturedMeshRenderer        mesh + UVs + texture + poses on the device -> {"rgba", "depth", "clipped"}
  TexturedMeshTemplates       drop-in for model.template_datasets[name], beside render.MeshTemplates
Vertex colours are IGNORED when a texture is given (BOP's textured models carry none).  Out of scope: anisotropic filtering,
several textures per model (a `texnumber` other than 0 is an error), vertex colour x texture modulation, OBJ / MTL files, and as in
render.py near-plane clipping, shading other than ambient and anti-aliasing.  There is no CPU fallback.
"""
import os

import numpy as np
import torch

from . import _lib, render

MAX_TEXTURE = 16384                                 # gigapose_texture.h: GPT_MAX_TEXTURE
MAX_UV = 32768.0                                    # gigapose_texture.h: GPT_MAX_UV
_texture = _lib.SideLibrary("libgigapose_texture.so", "gpt")
TEXTURE_LIB_PATH, lib, _call = _texture.path, _texture.lib, _texture.call


def mip_levels(Ht, Wt):
    return _texture.value("gpt_mip_levels", Ht, Wt)


def mip_texels(Ht, Wt):
    return _texture.value("gpt_mip_texels", Ht, Wt)


# ------------------------------------------------------------------------------------------------ loaders
_UV_NAMES = (("texture_u", "texture_v"), ("u", "v"), ("s", "t"))


def corner_uv_from_vertices(vertex_uv, faces):
    """Per-vertex UVs (V,2) gathered through the faces (F,3) -> per-corner UVs f32 (F,3,2)."""
    uv = np.asarray(vertex_uv, np.float32).reshape(-1, 2)
    return np.ascontiguousarray(uv[np.asarray(faces, np.int64).reshape(-1, 3)])


def load_textured_ply(path):
    """-> dict: vertices f32 (V,3), faces int32 (F,3), colours u8 (V,3) | None (all three as render.load_ply returns them),
    corner_uv f32 (F,3,2), texture_file (the name after `comment TextureFile`, as written) | None.  UVs come from the per-face
    list `texcoord` (six floats: u, v of the three corners) when the file has one, else from the per-vertex pair texture_u /
    texture_v (also u / v, s / t) gathered through the faces.  ValueError: no UVs at all, a texcoord list that does not hold six
    values, a `texnumber` other than 0 (several textures per model are out of scope), and whatever load_ply rejects."""
    path, comments, got = render.read_ply(path)
    vertices, faces, colours = render.ply_mesh(path, got)
    texture_file = None
    for ln in comments:
        w = ln.split(None, 2)
        if len(w) == 3 and w[1] == "TextureFile":
            texture_file = w[2].strip()
    face = got.get("face", {})
    if "texnumber" in face and len(faces) and np.any(np.asarray(face["texnumber"]) != 0):
        raise ValueError(f"load_textured_ply: {path}: a face has texnumber != 0: several textures per model are out of scope")
    corner_uv = None
    if "texcoord" in face:
        rows = face["texcoord"]
        if isinstance(rows, list):
            if any(len(r) != 6 for r in rows):
                raise ValueError(f"load_textured_ply: {path}: a texcoord list does not hold six values (u, v of three corners)")
            rows = np.asarray(rows, np.float32).reshape(-1, 6)
        if rows.ndim != 2 or (len(rows) and rows.shape[1] != 6) or len(rows) != len(faces):
            raise ValueError(f"load_textured_ply: {path}: a texcoord list does not hold six values (u, v of three corners)")
        corner_uv = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3, 2))
    else:
        vert = got["vertex"]
        pair = next((p for p in _UV_NAMES if p[0] in vert and p[1] in vert), None)
        if pair is None:
            raise ValueError(f"load_textured_ply: {path}: the file has no texture coordinates (texture_u / texture_v, u / v or s / t "
                             "per vertex, or a texcoord list per face)")
        corner_uv = corner_uv_from_vertices(np.stack([np.asarray(vert[pair[0]], np.float32), np.asarray(vert[pair[1]], np.float32)], axis=1), faces)
    return dict(vertices=vertices, faces=faces, colours=colours, corner_uv=corner_uv, texture_file=texture_file)


def load_texture(path):
    """Any PIL-readable image -> rgb u8 (Ht,Wt,3): alpha is dropped, grey and palette images are expanded.  ValueError: a 16-bit
    or float image (mode I;16, I, F), or a side beyond 16384."""
    from PIL import Image

    with Image.open(os.fspath(path)) as im:
        if im.mode.startswith("I") or im.mode == "F":
            raise ValueError(f"load_texture: {path}: mode {im.mode} (16-bit or float samples) is not supported: convert to 8 bits")
        rgb = np.array(im.convert("RGB"), dtype=np.uint8, order="C")
    _check_texture_shape(rgb.shape, "load_texture")
    return rgb


def _check_texture_shape(shape, who):
    if len(shape) != 3 or shape[2] != 3 or not (1 <= shape[0] <= MAX_TEXTURE and 1 <= shape[1] <= MAX_TEXTURE):
        raise ValueError(f"{who}: expected a texture (Ht, Wt, 3) with 1 <= Ht, Wt <= {MAX_TEXTURE}, got {tuple(shape)}")


# ------------------------------------------------------------------------------------------------ the two entry points
@torch.no_grad()
def build_mips(rgb):
    """gpt_build_mips: rgb u8 (Ht,Wt,3) on the device -> the pyramid, int32 (gpt_mip_texels(Ht, Wt),), holding the 32-bit texels
    R | G << 8 | B << 16 | 0xff << 24 of every level, level 0 first."""
    rgb = _lib.on_device(rgb, torch.uint8, (None, None, 3), "build_mips", "texture")
    _check_texture_shape(rgb.shape, "build_mips")
    Ht, Wt = rgb.shape[:2]
    pyramid = torch.empty(mip_texels(Ht, Wt), dtype=torch.int32, device=rgb.device)
    _call("gpt_build_mips", rgb, Ht, Wt, pyramid, _lib.stream_ptr())
    return pyramid


@torch.no_grad()
def resolve_textured(vis, xy, vdepth, faces, corner_uv, pyramid, size, out=None):
    """gpt_resolve: the keys of render.raster + corner_uv f32 (F,3,2) + the pyramid of a size = (Ht, Wt) texture -> rgba u8
    (N,H,W,4), depth f32 (N,H,W); `out` = (rgba, depth) are buffers to write into."""
    who = "resolve_textured"
    vis, xy, vdepth, faces, N, H, W, V, F = render.key_inputs(who, vis, xy, vdepth, faces)
    corner_uv = _lib.on_device(corner_uv, torch.float32, (F, 3, 2), who, "corner_uv")
    Ht, Wt = int(size[0]), int(size[1])
    _check_texture_shape((Ht, Wt, 3), who)
    pyramid = _lib.on_device(pyramid, torch.int32, (mip_texels(Ht, Wt),), who, "pyramid")
    rgba, depth = render.resolve_out(who, out, N, H, W, vis.device)
    _call("gpt_resolve", vis, xy, vdepth, V, faces, F, corner_uv, pyramid, Ht, Wt, N, H, W, rgba, depth, _lib.stream_ptr())
    return rgba, depth


# ------------------------------------------------------------------------------------------------ the renderer
class TexturedMeshRenderer(render.Renderer):
    """vertices f32 (V,3), faces int32 (F,3), corner_uv f32 (F,3,2), texture, poses f32 (N,4,4), all on the device -> rgba u8
    (N,H,W,4), depth f32 (N,H,W), clipped int32 (N,), as render.MeshRenderer returns them (same poses, K, pixel centres, znear).
    texture: rgb u8 (Ht,Wt,3), of which the pyramid is built once per call, or a pyramid built before, as (pyramid, (Ht, Wt)).
    The colour is the filtered texel alone: vertex colours are not an input."""
    who = "TexturedMeshRenderer"

    def __call__(self, vertices, faces, corner_uv, texture, poses, views_per_call=None, on_clipped="raise"):
        """Chunking, the clipped-view error and the one host synchronisation are MeshRenderer's."""
        return self._draw(vertices, faces, poses, views_per_call, on_clipped, corner_uv=corner_uv, texture=texture)

    def _prepare(self, vertices, faces, poses, corner_uv, texture):
        who = self.who
        corner_uv = _lib.on_device(corner_uv, torch.float32, (faces.shape[0], 3, 2), who, "corner_uv")
        if isinstance(texture, (tuple, list)):
            pyramid, size = texture
            size = (int(size[0]), int(size[1]))
            _check_texture_shape(size + (3,), who)
            pyramid = _lib.on_device(pyramid, torch.int32, (mip_texels(*size),), who, "pyramid")
        else:
            texture = _lib.on_device(texture, torch.uint8, (None, None, 3), who, "texture")
            _check_texture_shape(texture.shape, who)
            pyramid, size = build_mips(texture), tuple(texture.shape[:2])
        return faces, corner_uv, pyramid, size

    def _resolve_chunk(self, state, keys, pxy, pz, a, b, out):
        resolve_textured(keys, pxy, pz, *state, out=(out["rgba"][a:b], out["depth"][a:b]))


def _host_textured_mesh(mesh, texture, who):
    """-> vertices, faces, corner_uv, texture as host tensors."""
    base = None
    if isinstance(mesh, (str, os.PathLike)):
        base = os.path.dirname(os.path.abspath(os.fspath(mesh)))
        mesh = load_textured_ply(mesh)
    if not isinstance(mesh, dict) or not all(k in mesh for k in ("vertices", "faces", "corner_uv")):
        raise ValueError(f"{who}: the mesh must be a PLY path or a dict with vertices, faces and corner_uv")
    v, f, uv = (torch.from_numpy(render.host(mesh[k], t)) for k, t in (("vertices", np.float32), ("faces", np.int32), ("corner_uv", np.float32)))
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or tuple(uv.shape) != (f.shape[0], 3, 2):
        raise ValueError(f"{who}: expected vertices (V,3), faces (F,3), corner_uv (F,3,2), got {tuple(v.shape)}, {tuple(f.shape)}, {tuple(uv.shape)}")
    if len(f) and (int(f.min()) < 0 or int(f.max()) >= len(v)):
        raise ValueError(f"{who}: a face index is outside [0, {len(v)})")
    if texture is None:
        name = mesh.get("texture_file")
        if name is None:
            raise ValueError(f"{who}: no texture given and the mesh names none (`comment TextureFile` in the PLY)")
        texture = name if base is None or os.path.isabs(name) else os.path.join(base, name)
    if isinstance(texture, (str, os.PathLike)):
        texture = load_texture(texture)
    t = torch.from_numpy(render.host(texture, np.uint8))
    _check_texture_shape(t.shape, who)
    return v, f, uv, t


class TexturedMeshTemplates(render.TemplateSet):
    """Drop-in for `model.template_datasets[name]`, beside render.MeshTemplates: item i is the same PandasTensorCollection, .rgb
    (N,3,T,T) .mask (N,T,T) .K (3,3) .M (N,3,3) .poses (N,4,4) on the device.

    objects: list of (mesh, texture, poses) -- mesh a PLY path or a dict as load_textured_ply returns it; texture a path, an
    rgb array (Ht,Wt,3) or None to take the mesh's `texture_file` next to the PLY; poses (N,4,4) as for MeshTemplates.  Meshes
    and textures stay on the HOST; every __getitem__ uploads them, builds the pyramid, renders the N views on the device and hands
    the device renders to TemplateOnboarder: no render crosses PCIe.  Vertex colours in the mesh are ignored."""
    who = "TexturedMeshTemplates"

    def __init__(self, objects, K=None, device="cuda", target_size=224, H=480, W=640, znear=1e-3):
        super().__init__(objects, lambda K: TexturedMeshRenderer(H, W, K, znear), K, device, target_size)

    def _host_object(self, o, obj):
        if len(obj) != 3:
            raise ValueError(f"{self.who}: object {o}: expected (mesh, texture, poses)")
        mesh, texture, poses = obj
        return _host_textured_mesh(mesh, texture, f"{self.who}: object {o}"), poses

    def _render_object(self, mesh, poses):
        return self.renderer(*mesh, poses)
