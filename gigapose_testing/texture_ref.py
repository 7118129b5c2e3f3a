"""libgigapose_texture.so restated in numpy from the description in include/gigapose_texture.h (the arithmetic there is the
contract): the mip pyramid of 2 x 2 rounded means, perspective-correct UVs at a pixel and its two neighbours, the level of
detail from comparisons with powers of four, repeat-wrapped bilinear samples, the blend.  The GPU tests compare the kernels with
this bit for bit; tests/test_texture_host.py holds this file to exact rational arithmetic.

Like raster_ref it loops per (view, face) over the pixels a face owns, vectorised inside.  The keyword switches of `resolve` /
`inspect` / `build_mips` select deliberately WRONG renderers (affine interpolation, no UV swap, ...) that the host tests use to
show that their checks can fail; the defaults are the contract."""
import numpy as np

from . import raster_ref

MAX_TEXTURE = 16384
MAX_UV = 32768.0
CONTRACT = dict(interp="perspective", swap_uv=True, flip_v=True, wrap="repeat", l0_shift=0, rounding="floor")


# ------------------------------------------------------------------------------------------------ the pyramid
def mip_sizes(Ht, Wt, rounding="floor"):
    """[(H_l, W_l)] from level 0 down to 1 x 1.  rounding="ceil" is a mutant."""
    if not (1 <= Ht <= MAX_TEXTURE and 1 <= Wt <= MAX_TEXTURE):
        return []
    up = 0 if rounding == "floor" else 1
    sizes = [(int(Ht), int(Wt))]
    while sizes[-1] != (1, 1):
        h, w = sizes[-1]
        sizes.append((max(1, (h + up) >> 1), max(1, (w + up) >> 1)))
    return sizes


def mip_levels(Ht, Wt):
    return len(mip_sizes(Ht, Wt))


def mip_texels(Ht, Wt):
    return sum(h * w for h, w in mip_sizes(Ht, Wt))


def build_mips(rgb, rounding="floor"):
    """rgb (Ht,Wt,3) u8 -> the packed pyramid, uint32 (mip_texels,): R | G << 8 | B << 16 | 0xff << 24, level 0 first."""
    rgb = np.asarray(rgb, np.uint8)
    Ht, Wt = rgb.shape[:2]
    lev = np.concatenate([rgb.astype(np.uint32), np.full((Ht, Wt, 1), 255, np.uint32)], axis=2)
    out = []
    for h, w in mip_sizes(Ht, Wt, rounding):
        if (h, w) != lev.shape[:2]:
            sh, sw = lev.shape[:2]
            i, j = np.arange(h), np.arange(w)
            i0, i1 = np.minimum(2 * i, sh - 1), np.minimum(2 * i + 1, sh - 1)
            j0, j1 = np.minimum(2 * j, sw - 1), np.minimum(2 * j + 1, sw - 1)
            lev = (lev[i0][:, j0] + lev[i1][:, j0] + lev[i0][:, j1] + lev[i1][:, j1] + 2) >> 2
        out.append((lev[..., 0] | lev[..., 1] << 8 | lev[..., 2] << 16 | lev[..., 3] << 24).astype(np.uint32).reshape(-1))
    return np.concatenate(out)


def split_levels(pyramid, Ht, Wt, rounding="floor"):
    """The packed pyramid -> [u8 (H_l, W_l, 4)] (R, G, B, 255)."""
    pyramid = np.ascontiguousarray(np.asarray(pyramid).view(np.uint32).reshape(-1))
    out, o = [], 0
    for h, w in mip_sizes(Ht, Wt, rounding):
        out.append(pyramid[o:o + h * w].view(np.uint8).reshape(h, w, 4))
        o += h * w
    assert o == len(pyramid), f"the pyramid holds {len(pyramid)} texels, {Ht} x {Wt} needs {o}"
    return out


def pack_levels(levels):
    """[u8 (H_l, W_l, 3 or 4)] -> a packed pyramid (for pyramids written by hand)."""
    out = []
    for lev in levels:
        lev = np.asarray(lev, np.uint8).astype(np.uint32)
        out.append((lev[..., 0] | lev[..., 1] << 8 | lev[..., 2] << 16 | np.uint32(255) << 24).astype(np.uint32).reshape(-1))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ one face's pixels
def _within(x, bound):
    return (x >= -bound) & (x <= bound)


def _uv_at(e, r, cu, cv):
    t, q = raster_ref.weights(e, r)
    u = ((t[0] * cu[0] + t[1] * cu[1]) + t[2] * cu[2]) / q
    v = ((t[0] * cv[0] + t[1] * cv[1]) + t[2] * cv[2]) / q
    return q, u, v


def _face_lod(tri, face_row, cuv, e, dirs, r, sizes, swap_uv, l0_shift):
    """u, v, bad, rho2, l0, two, w of the pixels that face `tri` owns: e, dirs, r as raster_ref.drawn yields them."""
    swapped = tri[0][1] != int(face_row[1])
    order = (0, 2, 1) if (swapped and swap_uv) else (0, 1, 2)
    cu = [np.float64(cuv[k, 0]) for k in order]
    cv = [np.float64(cuv[k, 1]) for k in order]
    q, u, v = _uv_at(e, r, cu, cv)
    corners_ok = all(bool(_within(c, MAX_UV)) for c in cu + cv)
    bad = ~(_within(u, 2 * MAX_UV) & _within(v, 2 * MAX_UV)) | (not corners_ok)
    qx, ux, vx = _uv_at([e[k] - 256 * dirs[k][1] for k in range(3)], r, cu, cv)
    qy, uy, vy = _uv_at([e[k] + 256 * dirs[k][0] for k in range(3)], r, cu, cv)
    top = len(sizes) - 1
    Ht, Wt = np.float64(sizes[0][0]), np.float64(sizes[0][1])
    dsdx, dtdx, dsdy, dtdy = (ux - u) * Wt, (vx - v) * Ht, (uy - u) * Wt, (vy - v) * Ht
    ax, ay = dsdx * dsdx + dtdx * dtdx, dsdy * dsdy + dtdy * dtdy
    ok = ~((qx <= 0.0) | (qy <= 0.0)) & (ax == ax) & (ay == ay)
    rho2 = np.where(ay > ax, ay, ax)
    lv, p4 = np.zeros(len(u), np.int64), np.ones(len(u))
    for k in range(top):
        adv = (lv == k) & (p4 * 4.0 <= rho2)
        p4 = np.where(adv, p4 * 4.0, p4)
        lv = lv + adv
    if l0_shift:                                                    # mutant: one level too sharp
        low = lv > 0
        lv, p4 = lv - low, np.where(low, p4 / 4.0, p4)
    mag = ok & (rho2 < 1.0)
    l0 = np.where(ok, np.where(mag, 0, lv), top)
    two = ok & ~mag & (lv < top)
    w = np.where(two, (rho2 / p4 - 1.0) / 3.0, 0.0)
    return dict(u=u, v=v, bad=bad, rho2=np.where(ok, rho2, np.nan), l0=l0, two=two, w=w)


def _bilinear(lev, u, v, flip_v, wrap):
    hl, wl = lev.shape[:2]
    s = u * np.float64(wl) - 0.5
    t = ((1.0 - v) if flip_v else v) * np.float64(hl) - 0.5
    fs, ft = np.floor(s), np.floor(t)
    fx, fy = s - fs, t - ft
    gx, gy = 1.0 - fx, 1.0 - fy
    i0, j0 = fs.astype(np.int64), ft.astype(np.int64)
    if wrap == "repeat":
        i0, i1, j0, j1 = i0 % wl, (i0 + 1) % wl, j0 % hl, (j0 + 1) % hl
    else:                                                           # mutant: clamp to edge
        i0, i1, j0, j1 = np.clip(i0, 0, wl - 1), np.clip(i0 + 1, 0, wl - 1), np.clip(j0, 0, hl - 1), np.clip(j0 + 1, 0, hl - 1)
    c = lev[..., :3].astype(np.float64)
    c00, c10, c01, c11 = c[j0, i0], c[j0, i1], c[j1, i0], c[j1, i1]
    gx, fx, gy, fy = gx[:, None], fx[:, None], gy[:, None], fy[:, None]
    return (gx * c00 + fx * c10) * gy + (gx * c01 + fx * c11) * fy


def sample(levels, u, v, l0, two, w, flip_v=True, wrap="repeat"):
    """Trilinear sample at per-pixel (u, v, l0, two, w) -> float64 (n, 3) before the final rounding."""
    out = np.zeros((len(u), 3))
    for l in np.unique(l0):
        m = l0 == l
        out[m] = _bilinear(levels[l], u[m], v[m], flip_v, wrap)
        m2 = m & two
        if m2.any():
            B = _bilinear(levels[l + 1], u[m2], v[m2], flip_v, wrap)
            g = 1.0 - w[m2]
            out[m2] = g[:, None] * out[m2] + w[m2][:, None] * B
    return out


def _walk(vis, xy, depth, faces, corner_uv, Ht, Wt, interp, swap_uv, l0_shift, rounding):
    faces = np.asarray(faces)
    corner_uv = np.asarray(corner_uv, np.float32).reshape(len(faces), 3, 2)
    sizes = mip_sizes(Ht, Wt, rounding)
    with np.errstate(all="ignore"):
        for n, f, tri, py, px, e, dirs, r, z in raster_ref.drawn(vis, xy, depth, faces):
            if interp != "perspective":                             # mutant: screen-space weights
                r = [np.float64(1.0)] * 3
            yield n, f, py, px, z, _face_lod(tri, faces[f], corner_uv[f], e, dirs, r, sizes, swap_uv, l0_shift)


def inspect(vis, xy, depth, faces, corner_uv, Ht, Wt, interp="perspective", swap_uv=True, l0_shift=0, rounding="floor", **_):
    """Per pixel: u, v, rho2, w float64 (NaN where nothing is drawn; rho2 NaN where the level comes from a rule that has
    none), l0 int64 (-1 where nothing is drawn), two (l0 and l0 + 1 are blended), bad (bad UV), covered; each (N,H,W)."""
    shape = np.asarray(vis).shape
    out = {k: np.full(shape, np.nan) for k in ("u", "v", "rho2", "w")}
    out.update(l0=np.full(shape, -1, np.int64), two=np.zeros(shape, bool), bad=np.zeros(shape, bool), covered=np.zeros(shape, bool),
               face=np.full(shape, -1, np.int64))
    for n, f, py, px, _, d in _walk(vis, xy, depth, faces, corner_uv, Ht, Wt, interp, swap_uv, l0_shift, rounding):
        for k, a in d.items():
            out[k][n, py, px] = a
        out["covered"][n, py, px] = True
        out["face"][n, py, px] = f
    return out


def resolve(vis, xy, depth, faces, corner_uv, pyramid, Ht, Wt, interp="perspective", swap_uv=True, flip_v=True, wrap="repeat",
            l0_shift=0, rounding="floor"):
    """-> rgba (N,H,W,4) u8, zdepth (N,H,W) f32.  The keyword defaults are the contract; anything else is a mutant."""
    levels = split_levels(pyramid, Ht, Wt, rounding)
    N, H, W = np.asarray(vis).shape
    rgba = np.zeros((N, H, W, 4), np.uint8)
    zdepth = np.zeros((N, H, W), np.float32)
    for n, f, py, px, z, d in _walk(vis, xy, depth, faces, corner_uv, Ht, Wt, interp, swap_uv, l0_shift, rounding):
        good = ~d["bad"]
        colour = np.zeros((len(px), 3))
        if good.any():
            with np.errstate(all="ignore"):
                colour[good] = sample(levels, d["u"][good], d["v"][good], d["l0"][good], d["two"][good], d["w"][good], flip_v, wrap)
        rgba[n, py, px, :3] = np.clip(np.floor(colour + 0.5), 0.0, 255.0).astype(np.uint8)
        rgba[n, py, px, 3] = 255
        zdepth[n, py, px] = z
    return rgba, zdepth


def render(vertices, faces, corner_uv, texture, poses, K, H, W, znear, **variant):
    """texture: rgb (Ht,Wt,3) u8.  -> dict(xy, vdepth, vis, clipped, pyramid, rgba, depth)."""
    texture = np.asarray(texture, np.uint8)
    Ht, Wt = texture.shape[:2]
    xy, depth = raster_ref.project(vertices, poses, K, znear)
    vis, clipped = raster_ref.raster(xy, depth, faces, H, W)
    pyramid = build_mips(texture, variant.get("rounding", "floor"))
    rgba, zdepth = resolve(vis, xy, depth, faces, corner_uv, pyramid, Ht, Wt, **variant)
    return dict(xy=xy, vdepth=depth, vis=vis, clipped=clipped, pyramid=pyramid, rgba=rgba, depth=zdepth)


# ------------------------------------------------------------------------------------------------ textures, rgb (Ht,Wt,3) u8
def noise_texture(Ht, Wt, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (Ht, Wt, 3)).astype(np.uint8)


QUADRANTS = {"top_left": (230, 40, 40), "top_right": (40, 230, 40), "bottom_left": (40, 40, 230), "bottom_right": (230, 230, 40)}


def quadrant_card(Ht, Wt):
    """Four colours; "top_left" is u < 1/2, v > 1/2: image rows [0, Ht/2), columns [0, Wt/2)."""
    t = np.zeros((Ht, Wt, 3), np.uint8)
    t[:Ht // 2, :Wt // 2], t[:Ht // 2, Wt // 2:] = QUADRANTS["top_left"], QUADRANTS["top_right"]
    t[Ht // 2:, :Wt // 2], t[Ht // 2:, Wt // 2:] = QUADRANTS["bottom_left"], QUADRANTS["bottom_right"]
    return t


def ramp_u(Ht, Wt):
    """Column j holds rint(255 j / (Wt - 1)) in every channel: linear in u."""
    col = np.rint(255.0 * np.arange(Wt) / max(Wt - 1, 1)).astype(np.uint8)
    return np.repeat(np.repeat(col[None, :, None], Ht, axis=0), 3, axis=2)


def ramp_v(Ht, Wt):
    """Row i holds rint(255 (Ht - 1 - i) / (Ht - 1)): linear in v, dark at v = 0 (the bottom row)."""
    row = np.rint(255.0 * (Ht - 1 - np.arange(Ht)) / max(Ht - 1, 1)).astype(np.uint8)
    return np.repeat(np.repeat(row[:, None, None], Wt, axis=1), 3, axis=2)


def constant_texture(Ht, Wt, colour):
    return np.tile(np.asarray(colour, np.uint8)[None, None], (Ht, Wt, 1))
