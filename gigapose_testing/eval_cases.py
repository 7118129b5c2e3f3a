"""Inputs for the tests of pose scoring (gigapose_amd/evaluate.py, gigapose_testing/eval_ref.py), shared by the CPU and the GPU
suite: a set-based reading of the VSD rules in exact rational arithmetic, hand-built depth maps of dyadic values on which every
product and comparison is exact, and deterministic pose / symmetry data."""
from fractions import Fraction

import numpy as np


def vsd_by_sets(de, dg, dt, ray, delta, thr):
    """One pair: the visibility rules read as sets of pixels, distances as exact rationals -> [union, intersection, bad...]."""
    H, W = de.shape
    pixels = [(i, j) for i in range(H) for j in range(W)]

    def clean(d):
        return {p: (Fraction(float(d[p])) if np.isfinite(d[p]) and d[p] > 0 else Fraction(0)) for p in pixels}

    de, dg, dt = clean(de), clean(dg), clean(dt)
    r = {p: Fraction(float(ray[p])) for p in pixels}

    def visible(d):
        drawn = {p for p in pixels if d[p] > 0}
        in_front = {p for p in drawn if dt[p] > 0 and d[p] * r[p] - dt[p] * r[p] <= Fraction(delta)}
        no_measurement = {p for p in drawn if dt[p] == 0}
        return in_front | no_measurement

    vis_gt = visible(dg)
    vis_est = visible(de) | (vis_gt & {p for p in pixels if de[p] > 0})
    inter = vis_gt & vis_est
    out = [len(vis_gt | vis_est), len(inter)]
    for t in thr:
        out.append(len({p for p in inter if abs(dg[p] * r[p] - de[p] * r[p]) >= Fraction(float(t))}))
    return out


def hand_built_maps():
    """Dyadic depths and rays on a 6 x 8 frame, so that every product and comparison is exact in float64; every case of the
    rule occurs, several exactly on a boundary.  delta = 2, thresholds 0.5, 1, 3.125."""
    H, W = 6, 8
    ray = np.ones((H, W))
    ray[:, 4:] = 1.25                                                                # the right half: rays 1.25 x the depth
    de, dg, dt = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    dt[:] = 16.0
    dg[1:5, 1:7] = 12.0                                                              # the ground truth: in front of the scene
    de[2:6, 2:8] = 12.5                                                              # the estimate, shifted: cost 0.5 (left), 0.625 (right)
    de[2, 2], de[2, 3] = 12.0, 12.25                                                 #   ... and two pixels at cost 0 and 0.25
    dt[0, :] = 0.0                                                                   # a row without measurement
    dg[0, 0:3], de[0, 1:4] = 8.0, 9.0                                                #   ... where both count as visible; cost 1 (exactly thr[1])
    dt[3, 3], dt[3, 5] = 10.5, 10.0                                                  # an occluder: Dm - Dt = 1.5 / 2 on the left, 2.5 / 3.125 on the right
    dg[4, 1], dt[4, 1] = 12.0, 10.0                                                  # Dg - Dt exactly delta: visible
    dg[4, 2], dt[4, 2], de[4, 2] = 12.0, 11.0, 13.5                                  # est alone is occluded (2.5 > 2) but lies on a visible gt pixel
    de[5, 7], dt[5, 7] = 15.0, 12.0                                                  # De - Dt = 3.75 > delta: an estimate pixel fully hidden
    de[1, 6] = 14.5                                                                  # right half, on the ground truth: cost 2.5 * 1.25 = 3.125, exactly thr[2]
    de[1, 5] = 14.375                                                                #   ... and 2.375 * 1.25 = 2.96875, just below it
    dg[2, 1], de[2, 1], dt[5, 0] = -3.0, np.nan, np.inf                              # a negative, a NaN and an infinite depth: nothing
    dg[5, 0], dt[1, 1] = 7.0, -1.0
    return de, dg, dt, ray, 2.0, np.asarray([0.5, 1.0, 3.125])


def vsd_cases():
    de, dg, dt, ray, delta, thr = hand_built_maps()
    cases = [("every case", de, dg, dt)]
    zero = np.zeros_like(de)
    cases.append(("nothing visible", zero, zero, dt))
    cases.append(("estimate equal to ground truth", dg, dg, dt))
    near = np.full_like(dt, 4.0)
    cases.append(("both fully occluded", de, dg, near))
    cases.append(("estimate fully occluded", np.where(de > 0, np.float32(15.0), np.float32(0)), dg, np.where(dt > 0, np.float32(12.5), np.float32(0))))
    cases.append(("no measurement anywhere", de, dg, zero))
    return cases, ray, delta, thr




# ------------------------------------------------------------------------------------------------ poses and symmetries
HALF_TURN_X = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
HALF_TURN_Y = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
HALF_TURN_Z = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
CYLINDER = {"symmetries_discrete": [HALF_TURN_X], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}   # 630 transforms
K_CAMERA = np.asarray([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0])


def rigid(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def rotation(rs):
    q, r = np.linalg.qr(rs.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.linalg.det(q)


def small_motion(rs, angle, shift):
    """A rotation by `angle` about a random axis and a translation of length <= shift * sqrt(3)."""
    a = rs.standard_normal(3)
    a /= np.linalg.norm(a)
    c, s = np.cos(angle), np.sin(angle)
    cross = np.asarray([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return rigid(c * np.eye(3) + s * cross + (1 - c) * np.outer(a, a), rs.uniform(-shift, shift, 3))


def pose_case(seed, V, N, syms):
    """V random f32 vertices within +-60, N ground-truth poses 400..900 in front of the camera, estimates = the ground truth moved
    by a member of `syms` and a small motion (so that the minimum over the symmetries is not at an end by accident), one K per
    pair.  -> vertices, est, gt, K (N,9)."""
    rs = np.random.RandomState(seed)
    vertices = rs.uniform(-60, 60, (V, 3)).astype(np.float32)
    gt = np.stack([rigid(rotation(rs), (rs.uniform(-80, 80), rs.uniform(-60, 60), rs.uniform(400, 900))) for _ in range(N)])
    est = np.stack([g @ syms[rs.randint(len(syms))] @ small_motion(rs, 0.05, 3.0) for g in gt])
    K = np.tile(K_CAMERA, (N, 1))
    K[:, [0, 4]] *= rs.uniform(0.9, 1.1, (N, 1))
    K[:, [2, 5]] += rs.uniform(-5, 5, (N, 2))
    return vertices, est, gt, K
