"""The numpy restatement of include/gigapose_eval.h (libgigapose_eval.so, gigapose_amd/evaluate.py): the BOP-19 pose errors MSSD,
MSPD and VSD, operation by operation in float64 -- every product and sum below is one numpy element-wise operation (one rounding,
no fused multiply-add, no matmul / einsum whose summation order is numpy's business), in the order the header writes.  The
kernels must agree with it bit for bit (tests/test_gpu_eval.py); tests/test_eval_host.py holds it to exact rational arithmetic.

`variant` selects a deliberately WRONG scorer; the tests show that their checks reject each one:
  pose errors:  "mean" (mean over the vertices instead of the maximum), "min_per_vertex" (the minimum over the symmetries taken
                per vertex, then the maximum), "sym_left" (the symmetry applied on the estimate's left instead of the ground truth's right)
  vsd:          "z_depth" (the z-depth instead of the distance along the ray), "bop18" (the estimate's visibility without the
                ground truth's pixels), "inter_denominator" (the intersection instead of the union as the denominator)
"""
import numpy as np

F64 = np.float64


def sym_poses(gt, syms):
    """gt (N,4,4), syms (S,4,4) f64 -> G (N,S,3,4): rows 0..2 of gt[n] * syms[s], in the header's order."""
    g = np.asarray(gt, F64)[:, None, :3, :]                      # (N,1,3,4)
    m = np.asarray(syms, F64)[None]                              # (1,S,4,4)
    out = np.empty((g.shape[0], m.shape[1], 3, 4), F64)
    with np.errstate(all="ignore"):
        for j in range(4):
            col = (g[..., 0] * m[:, :, 0, j, None] + g[..., 1] * m[:, :, 1, j, None]) + g[..., 2] * m[:, :, 2, j, None]
            out[..., j] = col + g[..., 3] if j == 3 else col
    return out


def transform(P, x, y, z):
    """P (...,3,4) broadcast against the vertex coordinates (V,) -> X, Y, Z (...,V)."""
    return tuple(((P[..., i, 0, None] * x + P[..., i, 1, None] * y) + P[..., i, 2, None] * z) + P[..., i, 3, None] for i in range(3))


def project(K, X, Y, Z):
    """K (n,9), X, Y, Z (n,S,V) -> u, v."""
    k = [K[:, i, None, None] for i in range(6)]
    return ((k[0] * X + k[1] * Y) + k[2] * Z) / Z, ((k[3] * X + k[4] * Y) + k[5] * Z) / Z


def deviations(vertices, syms, est, gt, K, variant=None):
    """n pairs -> d2 (n,S,V), p2 (n,S,V), eZ (n,1,V), gZ (n,S,V)."""
    v = np.asarray(vertices, np.float32).astype(F64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    syms = np.asarray(syms, F64)
    if variant == "sym_left":
        G = np.stack([np.stack([(s @ g)[:3] for s in syms]) for g in gt])
    else:
        G = sym_poses(gt, syms)                                  # (n,S,3,4)
    with np.errstate(all="ignore"):
        eX, eY, eZ = transform(est[:, None, :3, :], x, y, z)     # (n,1,V)
        gX, gY, gZ = transform(G, x, y, z)                       # (n,S,V)
        dx, dy, dz = eX - gX, eY - gY, eZ - gZ
        d2 = (dx * dx + dy * dy) + dz * dz
        eu, ev = project(K, eX, eY, eZ)
        gu, gv = project(K, gX, gY, gZ)
        du, dv = eu - gu, ev - gv
        p2 = du * du + dv * dv
    return d2, p2, eZ, gZ


def mssd_mspd2(vertices, syms, est, gt, K, zmin=0.0, variant=None, elements_per_step=1 << 21):
    """vertices (V,3) f32, syms (S,4,4), est, gt (N,4,4), K (N,9) or (N,3,3) f64 -> mssd2 (N,), mspd2 (N,) f64: the squares.
    Vectorised over as many pairs as keep an intermediate array below `elements_per_step` elements."""
    est, gt = np.asarray(est, F64), np.asarray(gt, F64)
    N = len(est)
    K = np.asarray(K, F64).reshape(N, 9)
    out_d, out_p = np.empty(N, F64), np.empty(N, F64)
    step = max(1, elements_per_step // max(1, len(syms) * len(vertices)))
    for a in range(0, N, step):
        b = min(N, a + step)
        d2, p2, eZ, gZ = deviations(vertices, syms, est[a:b], gt[a:b], K[a:b], variant)
        with np.errstate(all="ignore"):
            if variant == "mean":
                md, mp = d2.mean(axis=2).min(axis=1), p2.mean(axis=2).min(axis=1)
            elif variant == "min_per_vertex":
                md, mp = d2.min(axis=1).max(axis=1), p2.min(axis=1).max(axis=1)
            else:
                md, mp = d2.max(axis=2).min(axis=1), p2.max(axis=2).min(axis=1)      # np.max lets a NaN through
            ok_d = np.isfinite(d2).all(axis=(1, 2))
            ok_p = np.isfinite(p2).all(axis=(1, 2)) & ~(eZ < zmin).any(axis=(1, 2)) & ~(gZ < zmin).any(axis=(1, 2))
        out_d[a:b], out_p[a:b] = np.where(ok_d, md, np.inf), np.where(ok_p, mp, np.inf)
    return out_d, out_p


def ray_map(K, H, W):
    """(H,W) f64: the length of the viewing ray through each pixel at unit depth."""
    K = np.asarray(K, F64).reshape(9)
    a = (np.arange(W, dtype=F64)[None, :] - K[2]) / K[0]
    b = (np.arange(H, dtype=F64)[:, None] - K[5]) / K[4]
    return np.sqrt((a * a + b * b) + 1.0)


def clean_depth(d):
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((d > 0) & np.isfinite(d), d, np.float32(0))


def vsd_counts(depth_est, depth_gt, depth_test, frame, ray, ray_index, delta, thr, variant=None):
    """depth_est, depth_gt (N,H,W) f32, depth_test (M,H,W) f32, frame (N,), ray (R,H,W) f64, ray_index (N,), thr (N,T) f64 ->
    counts (N, 2+T) int64 = union, intersection, bad[t]."""
    thr = np.asarray(thr, F64)
    N, T = thr.shape
    out = np.zeros((N, 2 + T), np.int64)
    for n in range(N):
        de, dg, dt = clean_depth(depth_est[n]), clean_depth(depth_gt[n]), clean_depth(depth_test[frame[n]])
        r = np.ones(de.shape, F64) if variant == "z_depth" else np.asarray(ray[ray_index[n]], F64)
        De, Dg, Dt = de.astype(F64) * r, dg.astype(F64) * r, dt.astype(F64) * r
        vis_gt = ((dg > 0) & (dt > 0) & ((Dg - Dt) <= delta)) | ((dg > 0) & (dt == 0))
        vis_est = ((de > 0) & (dt > 0) & ((De - Dt) <= delta)) | ((de > 0) & (dt == 0))
        if variant != "bop18":
            vis_est = vis_est | (vis_gt & (de > 0))
        inter = vis_gt & vis_est
        cost = np.abs(Dg - De)
        out[n, 0], out[n, 1] = (vis_gt | vis_est).sum(), inter.sum()
        for t in range(T):
            out[n, 2 + t] = (inter & (cost >= thr[n, t])).sum()
    return out


def vsd_from_counts(counts, variant=None):
    """counts (N, 2+T) -> e (N,T) f64: (bad + union - inter) / union, 1.0 where union = 0."""
    c = np.asarray(counts, np.int64)
    union, inter, bad = c[:, 0:1], c[:, 1:2], c[:, 2:]
    den = inter if variant == "inter_denominator" else union
    with np.errstate(all="ignore"):
        e = (bad + union - inter).astype(F64) / den.astype(F64)
    return np.where(den == 0, 1.0, e)
