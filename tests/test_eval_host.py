"""CPU: the host half of pose scoring (gigapose_amd/evaluate.py, libgigapose_eval.so, include/gigapose_eval.h).

The numpy restatement of the header (gigapose_testing/eval_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_eval.py); here it is held to something that cannot share its mistakes: exact rational arithmetic
(fractions.Fraction over the float64 inputs) for MSSD / MSPD, and a set-based reading of the visibility rules for VSD.  Six
subtly wrong scorers fail the same checks.  Beside that: symmetry_transforms, the greedy matching against a brute-force reading
of the rule on hand cases, the library against its header, and the argument validation of every entry point (no GPU needed)."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, evaluate, ingest, onboard, render
from gigapose_testing import eval_ref
from gigapose_testing.eval_cases import hand_built_maps, vsd_by_sets, vsd_cases
from gigapose_testing.symbols import exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = Fraction(1, 2 ** 53)


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------- the library and its header
def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gigapose_eval.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpe_[a-z0-9_]+)\s*\(", src)))


def test_eval_library_exports_exactly_its_header_and_no_symbol_of_the_other_libraries():
    names = declared_symbols()
    assert names == ["gpe_abi_version", "gpe_last_error", "gpe_mssd_mspd", "gpe_pose_workspace_bytes", "gpe_vsd_counts"]
    exported = exported_symbols(evaluate.EVAL_LIB_PATH)
    assert [n for n in exported if n.startswith("gpe_")] == names
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the eval library"
    lib = evaluate.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gpe_abi_version() >= 1
    for path in (_lib.LIB_PATH, _lib.PROBE_LIB_PATH, ingest.INGEST_LIB_PATH, onboard.ONBOARD_LIB_PATH, render.RENDER_LIB_PATH):
        assert not [n for n in exported_symbols(path) if n.startswith("gpe_")], path


def test_eval_argument_validation_of_the_library_needs_no_gpu():
    lib = evaluate.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    d = ctypes.c_double
    err = lib.gpe_last_error
    assert lib.gpe_mssd_mspd(null, 5, null, 2, null, null, null, 3, d(0.0), null, null, null, null) == -1
    assert b"gpe_mssd_mspd" in err() and b"null" in err()
    assert lib.gpe_mssd_mspd(one, 0, one, 2, one, one, one, 3, d(0.0), one, one, one, null) == -1          # V = 0
    assert b"bad sizes" in err()
    assert lib.gpe_mssd_mspd(one, 5, one, 0, one, one, one, 3, d(0.0), one, one, one, null) == -1          # S = 0
    assert b"bad sizes" in err() and b"S >= 1" in err()
    assert lib.gpe_mssd_mspd(one, 5, one, 2, one, one, one, 65536, d(0.0), one, one, one, null) == -1      # N > 65535
    assert lib.gpe_mssd_mspd(one, 5, one, 2, one, one, one, -1, d(0.0), one, one, one, null) == -1
    assert lib.gpe_mssd_mspd(one, 5, one, 2, one, one, one, 3, d(float("nan")), one, one, one, null) == -1
    assert b"zmin" in err()
    assert lib.gpe_mssd_mspd(one, 5, one, 2, one, one, one, 3, d(float("inf")), one, one, one, null) == -1
    assert lib.gpe_mssd_mspd(one, 5, one, 2, one, one, one, 3, d(0.0), one, one, ctypes.c_void_p(12), null) == -1
    assert b"aligned" in err()
    assert lib.gpe_mssd_mspd(null, 5, null, 2, null, null, null, 0, d(0.0), null, null, null, null) == 0   # N = 0: nothing to do

    def vsd(est=one, gt=one, N=2, test=one, M=2, frame=one, ray=one, R=1, ri=one, H=48, W=64, delta=15.0, thr=one, T=10, counts=one):
        return lib.gpe_vsd_counts(est, gt, N, test, M, frame, ray, R, ri, H, W, d(delta), thr, T, counts, null)

    assert vsd(est=null) == -1 and b"gpe_vsd_counts" in err() and b"null" in err()
    for kw in (dict(thr=null), dict(counts=null), dict(frame=null), dict(ri=null), dict(ray=null), dict(test=null), dict(gt=null)):
        assert vsd(**kw) == -1 and b"null" in err(), kw
    assert vsd(T=17) == -1 and b"T must be" in err()
    assert vsd(T=0) == -1 and b"T must be" in err()
    for kw in (dict(N=65536), dict(N=-1), dict(H=0), dict(W=-3), dict(H=65536, W=32768), dict(M=0), dict(R=0)):
        assert vsd(**kw) == -1 and b"bad sizes" in err(), kw
    assert vsd(delta=float("nan")) == -1 and b"delta" in err()
    assert vsd(counts=ctypes.c_void_p(12)) == -1 and b"aligned" in err()
    assert vsd(est=null, gt=null, test=null, frame=null, ray=null, ri=null, thr=null, counts=null, N=0) == 0

    assert lib.gpe_pose_workspace_bytes(1500, 630) == 1500 * 630 * 14 * 8
    assert lib.gpe_pose_workspace_bytes(65535, 2 ** 31 - 1) == 65535 * (2 ** 31 - 1) * 14 * 8              # size_t arithmetic
    assert lib.gpe_pose_workspace_bytes(-1, 5) == 0 and lib.gpe_pose_workspace_bytes(5, -1) == 0


def test_eval_argument_validation_of_the_python_layer_needs_no_gpu():
    v, s = torch.zeros(5, 3), torch.eye(4, dtype=torch.float64)[None]
    p, k = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1), torch.zeros(2, 9, dtype=torch.float64)
    f = evaluate.mssd_mspd
    with pytest.raises(ValueError, match="vertices"):
        f(v.double(), s, p, p, k)                                                    # dtype
    with pytest.raises(ValueError, match="vertices"):
        f(v[:, :2], s, p, p, k)                                                      # shape
    with pytest.raises(ValueError, match="must be a torch tensor"):
        f(v.numpy(), s, p, p, k)
    with pytest.raises(ValueError, match="syms"):
        f(v, s.float(), p, p, k)
    with pytest.raises(ValueError, match="gt"):
        f(v, s, p, p[:1], k)                                                         # est and gt differ in N
    with pytest.raises(ValueError, match="K"):
        f(v, s, p, p, k.reshape(2, 3, 3))
    with pytest.raises(ValueError, match="not contiguous"):
        f(v, s, p.transpose(1, 2), p, k)
    with pytest.raises(ValueError, match="not contiguous"):
        f(torch.zeros(3, 5).t(), s, p, p, k)
    with pytest.raises(ValueError, match="S = 0"):
        f(v, s[:0], p, p, k)
    with pytest.raises(ValueError, match="V = 0"):
        f(v[:0], s, p, p, k)
    with pytest.raises(ValueError, match="zmin"):
        f(v, s, p, p, k, zmin=float("nan"))
    with pytest.raises(ValueError, match="65535"):
        f(v, s, p[:1].expand(65536, 4, 4).contiguous(), p[:1].expand(65536, 4, 4).contiguous(), torch.zeros(65536, 9, dtype=torch.float64))
    with pytest.raises(ValueError, match="workspace is too small"):
        f(v, s, p, p, k, workspace=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        f(v, s, p, p, k)                                                             # everything right but the device

    de, dt = torch.zeros(2, 4, 6), torch.zeros(3, 4, 6)
    ray, thr = torch.ones(2, 4, 6, dtype=torch.float64), torch.ones(2, 10, dtype=torch.float64)
    fr, ri = np.asarray([0, 2]), np.asarray([1, 0])
    g = evaluate.vsd_counts
    with pytest.raises(ValueError, match="depth_est"):
        g(de.double(), de, dt, fr, ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match="depth_gt"):
        g(de, de[:1], dt, fr, ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match="depth_test"):
        g(de, de, dt[:, :3], fr, ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match="ray"):
        g(de, de, dt, fr, ray.float(), ri, 15.0, thr)
    with pytest.raises(ValueError, match="thr"):
        g(de, de, dt, fr, ray, ri, 15.0, thr[:1])
    with pytest.raises(ValueError, match="T = 17"):
        g(de, de, dt, fr, ray, ri, 15.0, torch.ones(2, 17, dtype=torch.float64))
    with pytest.raises(ValueError, match="T = 0"):
        g(de, de, dt, fr, ray, ri, 15.0, torch.ones(2, 0, dtype=torch.float64))
    with pytest.raises(ValueError, match="not contiguous"):
        g(torch.zeros(2, 6, 4).transpose(1, 2), de, dt, fr, ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match=r"frame index lies outside \[0, 3\)"):
        g(de, de, dt, np.asarray([0, 3]), ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match=r"frame index lies outside"):
        g(de, de, dt, torch.tensor([-1, 0]), ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match=r"ray_index index lies outside \[0, 2\)"):
        g(de, de, dt, fr, ray, np.asarray([2, 0]), 15.0, thr)
    with pytest.raises(ValueError, match="frame"):
        g(de, de, dt, np.asarray([0.0, 1.0]), ray, ri, 15.0, thr)                    # not integers
    with pytest.raises(ValueError, match="frame"):
        g(de, de, dt, fr[:1], ray, ri, 15.0, thr)
    with pytest.raises(ValueError, match="delta"):
        g(de, de, dt, fr, ray, ri, float("nan"), thr)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        g(de, de, dt, fr, ray, ri, 15.0, thr)

    eye = np.eye(4)[None].repeat(2, 0)
    K = np.asarray([[500.0, 0, 32], [0, 500.0, 24], [0, 0, 1]])
    with pytest.raises(ValueError, match="vertices"):
        evaluate.pose_errors(np.zeros((5, 2), np.float32), np.eye(4)[None], eye, eye, K)
    with pytest.raises(ValueError, match="gt"):
        evaluate.pose_errors(np.zeros((5, 3), np.float32), np.eye(4)[None], eye, eye[:1], K)
    with pytest.raises(ValueError, match="K"):
        evaluate.pose_errors(np.zeros((5, 3), np.float32), np.eye(4)[None], eye, eye, np.zeros((3, 3, 3)))
    with pytest.raises(ValueError, match="at least one vertex and one symmetry"):
        evaluate.pose_errors(np.zeros((5, 3), np.float32), np.zeros((0, 4, 4)), eye, eye, K)
    with pytest.raises(ValueError, match="dtype"):
        evaluate.pose_errors(np.zeros((5, 3), np.int32), np.eye(4)[None], eye, eye, K)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        evaluate.pose_errors(np.zeros((5, 3), np.float32), np.eye(4)[None], eye, eye, K, device="cpu")
    mesh = (np.zeros((5, 3), np.float32), np.zeros((2, 3), np.int32))
    depth = np.zeros((3, 48, 64), np.float32)
    with pytest.raises(ValueError, match="faces"):
        evaluate.vsd_errors((mesh[0], np.zeros((2, 4), np.int32)), eye, eye, K, depth, [0, 1], 10.0, H=48, W=64)
    with pytest.raises(ValueError, match="depth_test"):
        evaluate.vsd_errors(mesh, eye, eye, K, depth, [0, 1], 10.0, H=48, W=32)
    with pytest.raises(ValueError, match=r"frame index lies outside \[0, 3\)"):
        evaluate.vsd_errors(mesh, eye, eye, K, depth, [0, 3], 10.0, H=48, W=64)
    with pytest.raises(ValueError, match="17 taus"):
        evaluate.vsd_errors(mesh, eye, eye, K, depth, [0, 1], 10.0, taus=np.linspace(0.01, 0.5, 17), H=48, W=64)
    with pytest.raises(ValueError, match="diameter"):
        evaluate.vsd_errors(mesh, eye, eye, K, depth, [0, 1], [10.0, 11.0, 12.0], H=48, W=64)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        evaluate.vsd_errors(mesh, eye, eye, K, depth, [0, 1], 10.0, H=48, W=64, device="cpu")
    with pytest.raises(ValueError, match="no camera"):
        evaluate.PoseScorer({1: dict(vertices=mesh[0], faces=mesh[1], diameter=1.0)}, [dict(scene_id=1, im_id=2, obj_id=1, inst_count=1)], {},
                            {(1, 1): dict(cam_K=K, depth=depth[0])})
    with pytest.raises(ValueError, match="no model"):
        evaluate.PoseScorer({1: dict(vertices=mesh[0], faces=mesh[1], diameter=1.0)}, [dict(scene_id=1, im_id=1, obj_id=2, inst_count=1)], {},
                            {(1, 1): dict(cam_K=K, depth=depth[0])})


# ---------------------------------------------------------------------------------------------- MSSD / MSPD in exact arithmetic
def frac(a):
    return [Fraction(float(x)) for x in np.asarray(a, np.float64).reshape(-1)]


def exact_pose_errors(vertices, syms, est_n, gt_n, K_n):
    """One pair in rational arithmetic over the float64 inputs -> mssd2, mspd2 and the magnitudes the header's bound is written in:
    Be, Bg (the sums of absolute values behind a coordinate), Zmin (the smallest |Z| met), Ksum."""
    P, g, K = frac(est_n), frac(gt_n), frac(K_n)
    verts = [frac(v) + [Fraction(1)] for v in np.asarray(vertices, np.float32)]
    Be = Bg = Fraction(0)
    Zmin = None
    per_sym_d, per_sym_p = [], []
    for S in syms:
        S = frac(S)
        G = [[sum(g[4 * i + k] * S[4 * k + j] for k in range(3)) + (g[4 * i + 3] if j == 3 else 0) for j in range(4)] for i in range(3)]
        Gabs = [[sum(abs(g[4 * i + k]) * abs(S[4 * k + j]) for k in range(3)) + (abs(g[4 * i + 3]) if j == 3 else 0) for j in range(4)]
                for i in range(3)]
        ds, ps = [], []
        for x in verts:
            e = [sum(P[4 * i + j] * x[j] for j in range(4)) for i in range(3)]
            q = [sum(G[i][j] * x[j] for j in range(4)) for i in range(3)]
            Be = max(Be, max(sum(abs(P[4 * i + j]) * abs(x[j]) for j in range(4)) for i in range(3)))
            Bg = max(Bg, max(sum(Gabs[i][j] * abs(x[j]) for j in range(4)) for i in range(3)))
            Zmin = min(abs(e[2]), abs(q[2])) if Zmin is None else min(Zmin, abs(e[2]), abs(q[2]))
            ds.append(sum((a - b) ** 2 for a, b in zip(e, q)))
            pe = [(K[3 * r] * e[0] + K[3 * r + 1] * e[1] + K[3 * r + 2] * e[2]) / e[2] for r in range(2)]
            pg = [(K[3 * r] * q[0] + K[3 * r + 1] * q[1] + K[3 * r + 2] * q[2]) / q[2] for r in range(2)]
            ps.append(sum((a - b) ** 2 for a, b in zip(pe, pg)))
        per_sym_d.append(max(ds))
        per_sym_p.append(max(ps))
    Ksum = max(abs(K[0]) + abs(K[1]) + abs(K[2]), abs(K[3]) + abs(K[4]) + abs(K[5]))
    return min(per_sym_d), min(per_sym_p), dict(Be=Be, Bg=Bg, Zmin=Zmin, Ksum=Ksum)


def quarter_turns():
    """The 24 rotations by multiples of 90 degrees: signed permutation matrices of determinant +1."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            R = np.zeros((3, 3))
            for i, p in enumerate(perm):
                R[i, p] = -1.0 if signs >> i & 1 else 1.0
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    return out


def rigid(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def exact_case():
    """Inputs on which every operation of the written order is exact in float64, the divisions included: vertices at corners of
    the cube (+-2)^3 (an asymmetric subset), rotations by multiples of 90 degrees, symmetry transforms without translation, dyadic
    translations with tz = 6 -- so every Z is 4 or 8 -- and a dyadic K."""
    vertices = np.asarray([(2, 2, 2), (-2, 2, 2), (2, -2, 2), (2, 2, -2), (-2, -2, 2), (-2, 2, -2)], np.float32)
    turns = quarter_turns()
    assert len(turns) == 24
    syms = np.stack([rigid(np.eye(3), (0, 0, 0)), rigid(turns[5], (0, 0, 0)), rigid(turns[10], (0, 0, 0)), rigid(turns[17], (0, 0, 0))])
    rs = np.random.RandomState(7)
    est, gt = [], []
    for n in range(12):
        a, b = turns[rs.randint(24)], turns[rs.randint(24)]
        if n % 3 == 0:
            b = a @ syms[1 + n // 3 % 3][:3, :3].T                                   # the estimate is the ground truth moved by a symmetry
        est.append(rigid(a, (rs.randint(-8, 9) / 4.0, rs.randint(-8, 9) / 8.0, 6.0)))
        gt.append(rigid(b, (rs.randint(-8, 9) / 4.0, rs.randint(-8, 9) / 8.0, 6.0)))
    K = np.tile(np.asarray([512.0, 0.0, 320.5, 0.0, 256.0, 240.25, 0.0, 0.0, 1.0]), (12, 1))
    K[::2, 1] = 0.5                                                                  # a skew: K1 is read
    return vertices, syms, np.stack(est), np.stack(gt), K


def exact_mismatches(variant):
    """Pairs of the exact case on which the scorer differs from the rational value: (in mssd2, in mspd2)."""
    v, syms, est, gt, K = exact_case()
    d2, p2 = eval_ref.mssd_mspd2(v, syms, est, gt, K, zmin=0.0, variant=variant)
    bad_d = bad_p = 0
    for n in range(len(est)):
        want_d, want_p, _ = exact_pose_errors(v, syms, est[n], gt[n], K[n])
        bad_d += not np.isfinite(d2[n]) or Fraction(float(d2[n])) != want_d
        bad_p += not np.isfinite(p2[n]) or Fraction(float(p2[n])) != want_p
    return bad_d, bad_p


def test_restatement_equals_exact_arithmetic_where_every_operation_is_exact():
    assert exact_mismatches(None) == (0, 0)
    v, syms, est, gt, K = exact_case()
    d2, p2 = eval_ref.mssd_mspd2(v, syms, est, gt, K)
    assert (d2 > 0).sum() >= 6 and (p2 > 0).sum() >= 6 and len(set(d2.tolist())) >= 4       # the case is not degenerate


@pytest.mark.parametrize("variant", ["mean", "min_per_vertex", "sym_left"])
def test_the_exact_check_rejects_wrong_pose_scorers(variant):
    """The mean over the vertices instead of the maximum; the minimum over the symmetries taken per vertex (a lower bound of the
    error that no single symmetry reaches); the symmetry applied on the estimate's left (a motion of the camera, not of the
    object).  Each differs from the rational value on several of the twelve pairs, in both errors."""
    bad_d, bad_p = exact_mismatches(variant)
    assert bad_d >= 3 and bad_p >= 3


def random_rotation(rs):
    q, r = np.linalg.qr(rs.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.linalg.det(q)


def test_restatement_stays_within_the_header_bound_on_random_rotations():
    """Random rotations, f32 vertices of magnitude ~60, objects at z ~ 400: nothing is exact.  The bound is the one
    include/gigapose_eval.h derives from the operation count of the written order, with u = 2^-53, gamma_k = k u / (1 - k u):
      a coordinate of e: a 4-term dot product, <= 4 roundings on a term              -> gamma_4 * Be
      a coordinate of g: an entry of G (gamma_4), then the same dot product          -> gamma_8 * Bg
      a difference: one more rounding, |difference| <= B = Be + Bg                   -> eps = gamma_9 * B
      d2: 3 products, 2 sums                                                         -> 3 B^2 (2 gamma_9 + gamma_9^2 + gamma_3 (1 + gamma_9)^2)
      a numerator: a 3-term dot product of coordinates carrying gamma_8              -> gamma_11 * Bn, Bn = Ksum * max(Be, Bg)
      u, v: divided by |Z| >= Zlow and rounded once; U = Bn / Zlow, rho = max(Be, Bg) / Zlow   -> eta = U (gamma_12 + gamma_8 rho)
      a pixel difference: |.| <= D = 2 U                                             -> eps_p = 2 U (gamma_13 + gamma_8 rho)
      p2: 2 products, 1 sum                                                          -> 2 (2 D eps_p + eps_p^2) + 2 gamma_2 (D + eps_p)^2
    with Zlow = the smallest exact |Z| minus gamma_8 * max(Be, Bg).  Be, Bg, Zlow are computed in rational arithmetic from the
    inputs; maximum and minimum are exact, so the per-point bounds hold for the results.  Nothing here is fitted to the
    restatement's actual error (which is recorded to be far below: the bound is a worst case)."""
    rs = np.random.RandomState(11)
    V, S, N = 12, 3, 4
    vertices = (rs.uniform(-60, 60, (V, 3))).astype(np.float32)
    syms = np.stack([np.eye(4)] + [rigid(random_rotation(rs), rs.uniform(-5, 5, 3)) for _ in range(S - 1)])
    est = np.stack([rigid(random_rotation(rs), (rs.uniform(-50, 50), rs.uniform(-50, 50), rs.uniform(350, 450))) for _ in range(N)])
    gt = np.stack([rigid(random_rotation(rs), (rs.uniform(-50, 50), rs.uniform(-50, 50), rs.uniform(350, 450))) for _ in range(N)])
    gt[0] = est[0] @ np.linalg.inv(syms[1])                                          # one pair that a symmetry explains, to rounding
    K = np.tile(np.asarray([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0]), (N, 1))
    d2, p2 = eval_ref.mssd_mspd2(vertices, syms, est, gt, K)
    worst = [Fraction(0), Fraction(0)]
    outside = {variant: [0, 0] for variant in ("mean", "min_per_vertex", "sym_left")}
    for n in range(N):
        want_d, want_p, m = exact_pose_errors(vertices, syms, est[n], gt[n], K[n])
        B, Bmax = m["Be"] + m["Bg"], max(m["Be"], m["Bg"])
        bound_d = 3 * B * B * (2 * gamma(9) + gamma(9) ** 2 + gamma(3) * (1 + gamma(9)) ** 2)
        Zlow = m["Zmin"] - gamma(8) * Bmax
        assert Zlow > 100
        Uu, rho = m["Ksum"] * Bmax / Zlow, Bmax / Zlow
        D, eps_p = 2 * Uu, 2 * Uu * (gamma(13) + gamma(8) * rho)
        bound_p = 2 * (2 * D * eps_p + eps_p ** 2) + 2 * gamma(2) * (D + eps_p) ** 2
        err_d, err_p = abs(Fraction(float(d2[n])) - want_d), abs(Fraction(float(p2[n])) - want_p)
        assert err_d <= bound_d, (n, float(err_d), float(bound_d))
        assert err_p <= bound_p, (n, float(err_p), float(bound_p))
        assert bound_d < 1e-6 and bound_p < 1e-4                                     # the bound itself says something: errors are ~1e3 .. 1e5
        worst = [max(worst[0], err_d / bound_d), max(worst[1], err_p / bound_p)]
        for variant in ("mean", "min_per_vertex", "sym_left"):
            wd, wp = eval_ref.mssd_mspd2(vertices, syms, est[n:n + 1], gt[n:n + 1], K[n:n + 1], variant=variant)
            outside[variant][0] += not np.isfinite(wd[0]) or abs(Fraction(float(wd[0])) - want_d) > bound_d
            outside[variant][1] += not np.isfinite(wp[0]) or abs(Fraction(float(wp[0])) - want_p) > bound_p
    assert all(d >= 2 and p >= 2 for d, p in outside.values()), outside              # the bound rejects the wrong scorers too
    assert worst[0] < 1 and worst[1] < 1
    assert float(want_d) > 1.0 and math.sqrt(d2[0]) < 1e-9                            # pair 0 is explained by symmetry 1; the others are not


def test_restatement_bad_inputs_give_infinity_for_that_pair_only():
    v, syms, est, gt, K = exact_case()
    est, gt = est[:4].copy(), gt[:4].copy()
    base_d, base_p = eval_ref.mssd_mspd2(v, syms, est, gt, K[:4])
    e2 = est.copy()
    e2[1, 0, 3] = np.inf
    d2, p2 = eval_ref.mssd_mspd2(v, syms, e2, gt, K[:4])
    assert np.isinf(d2[1]) and np.isinf(p2[1]) and (np.delete(d2, 1) == np.delete(base_d, 1)).all() and (np.delete(p2, 1) == np.delete(base_p, 1)).all()
    g2 = gt.copy()
    g2[2, 2, 3] = -6.0                                                               # the ground truth behind the camera: Z = -4, -8
    d2, p2 = eval_ref.mssd_mspd2(v, syms, est, g2, K[:4])
    assert np.isfinite(d2).all() and np.isinf(p2[2]) and np.isfinite(np.delete(p2, 2)).all()
    d2, p2 = eval_ref.mssd_mspd2(v, syms, est, gt, K[:4], zmin=5.0)                  # Z = 4 is met in every pair
    assert np.isinf(p2).all() and (d2 == base_d).all()
    vn = v.copy()
    vn[3, 1] = np.nan
    d2, p2 = eval_ref.mssd_mspd2(vn, syms, est, gt, K[:4])
    assert np.isinf(d2).all() and np.isinf(p2).all()


# ---------------------------------------------------------------------------------------------- VSD against sets of pixels
def test_hand_built_maps_hold_every_case():
    de, dg, dt, ray, delta, thr = hand_built_maps()
    want = vsd_by_sets(de, dg, dt, ray, delta, thr)
    got = eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None])[0].tolist()
    assert got == want
    assert want[0] > want[1] > want[2] > want[3] > want[4] > 0                       # union > inter > bad at 0.5 > at 1 > at 3 > 0


def test_restatement_equals_the_set_reading_on_hand_built_maps():
    cases, ray, delta, thr = vsd_cases()
    for name, de, dg, dt in cases:
        want = vsd_by_sets(de, dg, dt, ray, delta, thr)
        got = eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None])[0].tolist()
        assert got == want, name
    name, de, dg, dt = cases[1]
    c = eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None])
    assert c[0, 0] == 0 and eval_ref.vsd_from_counts(c).tolist() == [[1.0, 1.0, 1.0]]
    name, de, dg, dt = cases[2]
    c = eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None])
    assert c[0, 0] == c[0, 1] > 0 and eval_ref.vsd_from_counts(c).tolist() == [[0.0, 0.0, 0.0]]
    name, de, dg, dt = cases[4]
    c = eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None])
    assert c[0, 1] < c[0, 0]                                                         # what is left of it: the row without measurement
    # mixed indices: two frames, two ray maps
    _, de, dg, dt = cases[0]
    stack_t, stack_r = np.stack([np.zeros_like(dt), dt]), np.stack([np.ones_like(ray), ray])
    c = eval_ref.vsd_counts(np.stack([de, de, de]), np.stack([dg, dg, dg]), stack_t, [1, 0, 1], stack_r, [1, 1, 0], delta, np.tile(thr, (3, 1)))
    assert c[0].tolist() == vsd_by_sets(de, dg, dt, ray, delta, thr)
    assert c[1].tolist() == vsd_by_sets(de, dg, stack_t[0], ray, delta, thr)
    assert c[2].tolist() == vsd_by_sets(de, dg, dt, stack_r[0], delta, thr)
    assert len({tuple(r) for r in c.tolist()}) == 3


@pytest.mark.parametrize("variant", ["z_depth", "bop18", "inter_denominator"])
def test_the_set_check_rejects_wrong_vsd_scorers(variant):
    """The z-depth instead of the distance along the ray (the right half of the frame has rays of 1.25); the bop18 visibility
    (an estimate pixel that is occluded on its own but lies on a visible ground-truth pixel is lost); the intersection as the
    denominator."""
    cases, ray, delta, thr = vsd_cases()
    name, de, dg, dt = cases[0]
    want = vsd_by_sets(de, dg, dt, ray, delta, thr)
    want_e = [Fraction(b + want[0] - want[1], want[0]) for b in want[2:]]
    counts = eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None], variant=variant)
    e = eval_ref.vsd_from_counts(counts, variant=variant)[0]
    right = eval_ref.vsd_from_counts(eval_ref.vsd_counts(de[None], dg[None], dt[None], [0], ray[None], [0], delta, thr[None]))[0]
    assert [float(w) for w in want_e] == right.tolist()
    if variant == "inter_denominator":
        assert counts[0].tolist() == want
    else:
        assert counts[0].tolist() != want
    assert any(float(w) != g for w, g in zip(want_e, e.tolist()))


def test_ray_map_is_the_distance_of_the_unit_depth_point():
    K = np.asarray([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    for f in (evaluate.ray_map, eval_ref.ray_map):
        r = f(K, 48, 64)
        assert r.shape == (48, 64) and r.dtype == np.float64
        for py, px in ((0, 0), (47, 63), (20, 33)):
            p = np.linalg.inv(K) @ np.asarray([px, py, 1.0])
            assert abs(r[py, px] - np.linalg.norm(p)) < 1e-14
    np.testing.assert_array_equal(evaluate.ray_map(K, 48, 64), eval_ref.ray_map(K, 48, 64))
    np.testing.assert_array_equal(evaluate.vsd_from_counts([[10, 6, 3, 0], [0, 0, 0, 0]]), [[0.7, 0.4], [1.0, 1.0]])


# ---------------------------------------------------------------------------------------------- symmetry_transforms
HALF_TURN_Z = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def closed_under_composition(syms, diameter, left=None):
    """Every product of two members is a member, to 1e-12 of the diameter in the position of a point at the diameter's distance
    (rotation entries are weighed by the diameter).  `left`: the left factors to try (default: all)."""
    flat = syms.reshape(len(syms), 16)
    worst = 0.0
    for a in syms if left is None else syms[left]:
        prod = (a[None] @ syms).reshape(len(syms), 16)
        scale = np.asarray([diameter] * 3 + [1.0] + [diameter] * 3 + [1.0] + [diameter] * 3 + [1.0] + [1.0] * 4)
        dist = np.abs((prod[:, None, :] - flat[None, :, :]) * scale).max(axis=2).min(axis=1)
        worst = max(worst, float(dist.max()))
    return worst <= 1e-12 * diameter, worst


def test_symmetry_transform_counts_and_order():
    cont = [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]
    for info, n in (({}, 1), ({"symmetries_discrete": [HALF_TURN_Z]}, 2), ({"symmetries_continuous": cont}, 315),
                    ({"symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]], "symmetries_continuous": cont}, 630)):
        s = evaluate.symmetry_transforms(info)
        assert s.shape == (n, 4, 4) and s.dtype == np.float64 and s.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(s[0], np.eye(4))
        np.testing.assert_array_equal(s[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))
        assert np.abs(s[:, :3, :3] @ s[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
        assert np.abs(np.linalg.det(s[:, :3, :3]) - 1).max() < 1e-14
    assert evaluate.symmetry_transforms({"symmetries_continuous": cont}, max_sym_disc_step=0.1).shape[0] == 32
    with pytest.raises(ValueError):
        evaluate.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]})
    with pytest.raises(ValueError):
        evaluate.symmetry_transforms({"symmetries_discrete": [[1, 0, 0]]})


def test_symmetry_sets_are_closed_under_composition():
    diameter = 120.0
    quarter = [0, -1, 0, 30, 1, 0, 0, -10, 0, 0, 1, 0, 0, 0, 0, 1]                   # a quarter turn about the axis through (20, 10, .)
    group = [np.linalg.matrix_power(np.asarray(quarter, np.float64).reshape(4, 4), k).reshape(-1).tolist() for k in (1, 2, 3)]
    s = evaluate.symmetry_transforms({"symmetries_discrete": group})
    assert len(s) == 4
    ok, worst = closed_under_composition(s, diameter)
    assert ok, worst
    ok, _ = closed_under_composition(evaluate.symmetry_transforms({"symmetries_discrete": group[:1]}), diameter)
    assert not ok                                                                    # a quarter turn alone is no group: the check sees it
    axis = {"axis": [1.0, 2.0, -2.0], "offset": [5.0, -3.0, 12.0]}                   # not normalised, off the origin
    s = evaluate.symmetry_transforms({"symmetries_continuous": [axis]})
    ok, worst = closed_under_composition(s, diameter, left=[0, 1, 2, 100, 157, 158, 313, 314])
    assert ok, worst
    p = np.asarray([5.0, -3.0, 12.0]) + 7.5 * np.asarray([1.0, 2.0, -2.0]) / 3.0     # a point on the axis stays where it is
    assert np.abs(s[:, :3, :3] @ p + s[:, :3, 3] - p).max() < 1e-12
    flip = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]                         # half turn about x, with the z axis: a cylinder's group
    s = evaluate.symmetry_transforms({"symmetries_discrete": [flip], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    ok, worst = closed_under_composition(s, diameter, left=[0, 1, 157, 314, 315, 316, 500, 629])   # both cosets on the left
    assert len(s) == 630 and ok, worst


def test_a_pose_moved_by_a_symmetry_scores_zero():
    """est = gt * sym for every member: mssd = mspd = 0 to rounding (1e-9 of a diameter of 120, 1e-9 px), through the restatement."""
    rs = np.random.RandomState(3)
    flip = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
    syms = evaluate.symmetry_transforms({"symmetries_discrete": [flip], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]},
                                        max_sym_disc_step=0.05)
    assert len(syms) == 126
    vertices = rs.uniform(-60, 60, (9, 3)).astype(np.float32)
    gt = rigid(random_rotation(rs), (20.0, -30.0, 600.0))
    est = gt[None] @ syms
    K = np.asarray([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0])
    d2, p2 = eval_ref.mssd_mspd2(vertices, syms, est, np.tile(gt, (len(syms), 1, 1)), np.tile(K, (len(syms), 1)))
    assert np.sqrt(d2).max() < 1e-9 * 120 and np.sqrt(p2).max() < 1e-9
    d2, p2 = eval_ref.mssd_mspd2(vertices, syms[:1], est, np.tile(gt, (len(syms), 1, 1)), np.tile(K, (len(syms), 1)))
    assert np.sqrt(d2[1:]).min() > 1.0                                               # without the set the same poses are errors


# ---------------------------------------------------------------------------------------------- matching and recall
def brute_force_matches(errors, threshold):
    """The rule read literally: estimates in the given (descending score) order; each looks at every ground truth nobody has
    taken, picks the one with the smallest error, and takes it if that error is below the threshold."""
    taken = []
    for row in errors:
        best = None
        for g, err in enumerate(row):
            if g in taken:
                continue
            if best is None or err < row[best]:
                best = g
        if best is not None and row[best] < threshold:
            taken.append(best)
    return len(taken)


MATCH_CASES = [
    # (errors: estimates in descending score x ground truths, threshold, matched ground truths) -- the counts are worked by hand
    ("one of each, below", [[0.3]], 0.5, 1),
    ("one of each, exactly the threshold: not below", [[0.5]], 0.5, 0),
    ("no estimate", np.zeros((0, 2)), 0.5, 0),
    ("no ground truth", np.zeros((2, 0)), 0.5, 0),
    ("two instances, each estimate nearest its own", [[0.1, 0.9], [0.8, 0.2]], 0.5, 2),
    ("the first estimate takes the second ground truth, which the second wanted too", [[0.4, 0.1], [0.9, 0.2]], 0.5, 1),
    ("the same, and the second falls back on the first ground truth", [[0.4, 0.1], [0.3, 0.2]], 0.5, 2),
    ("an estimate better for the second ground truth leaves the first to the next", [[0.45, 0.05], [0.1, 0.01]], 0.5, 2),
    ("the best estimate fails; a worse-scored one matches", [[0.9, 0.8], [0.1, 0.7]], 0.5, 1),
    ("a tie in error: the lower index, so the second still finds one", [[0.2, 0.2], [0.9, 0.3]], 0.5, 2),
    ("three estimates for two ground truths", [[0.6, 0.7], [0.1, 0.2], [0.3, 0.1]], 0.5, 2),
    ("greedy is not optimal: the first takes what the second needed", [[0.1, 0.2], [0.3, 0.9]], 0.25, 1),
    ("an infinite error never matches", [[np.inf, np.inf], [0.1, np.inf]], 0.5, 1),
]


@pytest.mark.parametrize("name,errors,threshold,want", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_greedy_matching_on_hand_cases(name, errors, threshold, want):
    errors = np.asarray(errors, np.float64)
    assert evaluate.match_greedy(errors, threshold) == want
    assert brute_force_matches(errors.tolist(), threshold) == want


def test_greedy_matching_equals_the_brute_force_reading_on_random_cases():
    rs = np.random.RandomState(5)
    for _ in range(300):
        E, G = rs.randint(0, 5), rs.randint(0, 4)
        errors = np.round(rs.uniform(0, 1, (E, G)), 1)                               # one decimal: ties are frequent
        for th in (0.25, 0.5, 0.75):
            assert evaluate.match_greedy(errors, th) == brute_force_matches(errors.tolist(), th)


def scorer_without_gpu(targets, gts):
    mesh = dict(vertices=np.zeros((3, 3), np.float32), faces=np.zeros((1, 3), np.int32), diameter=100.0)
    cams = {(1, i): dict(cam_K=[500.0, 0, 32, 0, 500.0, 24, 0, 0, 1], depth=np.zeros((48, 64), np.float32)) for i in (1, 2)}
    return evaluate.PoseScorer({1: mesh, 2: mesh}, targets, gts, cams)


def test_scorer_keeps_the_highest_scored_estimates_of_each_target():
    def est(im, obj, score, tag):
        return dict(scene_id=1, im_id=im, obj_id=obj, score=score, R=np.eye(3), t=np.asarray([tag, 0.0, 1.0]))

    def gt(obj, tag):
        return dict(obj_id=obj, cam_R_m2c=np.eye(3).reshape(-1), cam_t_m2c=[tag, 0, 1])

    targets = [dict(scene_id=1, im_id=1, obj_id=1, inst_count=2), dict(scene_id=1, im_id=1, obj_id=2, inst_count=1),
               dict(scene_id=1, im_id=2, obj_id=1, inst_count=1)]
    gts = {(1, 1): [gt(1, 10), gt(2, 20), gt(1, 11)], (1, 2): [gt(2, 30)]}
    ests = [est(1, 1, 0.5, 0), est(1, 1, 0.9, 1), est(1, 1, 0.5, 2), est(1, 1, 0.7, 3), est(1, 2, 0.1, 4), est(2, 2, 0.9, 5), est(3, 1, 0.9, 6)]
    groups = scorer_without_gpu(targets, gts).pairs(ests)
    assert [[int(e["t"][0]) for e in kept] for _, kept, _ in groups] == [[1, 3], [4], []]      # inst_count < the number of estimates
    assert [[int(g["cam_t_m2c"][0]) for g in g_] for _, _, g_ in groups] == [[10, 11], [20], []]
    targets[0]["inst_count"] = 4
    groups = scorer_without_gpu(targets, gts).pairs(ests)
    assert [int(e["t"][0]) for e in groups[0][1]] == [1, 3, 0, 2]                               # a tie in score: file order


def test_recall_from_errors_against_the_brute_force_reading():
    """Two targets of different diameters, hand-made errors: the recalls per threshold are the brute-force matches over the ground
    truths counted; the averages are their means."""
    rs = np.random.RandomState(9)
    T = 10
    per_target = []
    for obj, E, G in ((1, 3, 2), (2, 1, 1), (1, 0, 2), (2, 2, 0)):
        per_target.append((dict(obj_id=obj), dict(mssd=rs.uniform(0, 60, (E, G)), mspd=rs.uniform(0, 120, (E, G)),
                                                  vsd=np.round(rs.uniform(0, 1, (E, G, T)), 2), clipped=np.zeros((E, G), bool))))
    diam = {1: 100.0, 2: 60.0}
    out = evaluate.recall_from_errors(per_target, diam, W=1280)
    assert out["targets"] == 5 and out["clipped"] == 0
    ths = [0.05 * i for i in range(1, 11)]
    for i in range(10):
        want = sum(brute_force_matches(e["mssd"].tolist(), evaluate.CORRECT_THS[i] * diam[t["obj_id"]]) for t, e in per_target) / 5
        assert out["recall_mssd"][i] == want and abs(evaluate.CORRECT_THS[i] - ths[i]) < 1e-15
        want = sum(brute_force_matches(e["mspd"].tolist(), 5.0 * (i + 1) * 2.0) for t, e in per_target) / 5       # r = 1280 / 640
        assert out["recall_mspd"][i] == want
        for k in range(T):
            want = sum(brute_force_matches(e["vsd"][:, :, k].tolist(), evaluate.CORRECT_THS[i]) for t, e in per_target) / 5
            assert out["recall_vsd"][k][i] == want
    assert 0 < out["ar_mssd"] < 1 and 0 < out["ar_mspd"] < 1 and 0 < out["ar_vsd"] < 1
    assert out["ar_mssd"] == float(np.mean(out["recall_mssd"])) and out["ar_vsd"] == float(np.mean(out["recall_vsd"]))
    assert abs(out["ar"] - (out["ar_mssd"] + out["ar_mspd"] + out["ar_vsd"]) / 3) < 1e-15


def test_read_estimates_reads_what_inout_writes(tmp_path):
    from gigapose_amd import inout
    from gigapose_testing import synthetic as syn

    batches = syn.prediction_batches(4, n_batches=2, k=3)
    for b, d in enumerate(batches):
        np.savez(str(tmp_path / f"{b}.npz"), **d)
    paths = inout.save_predictions_from_batched_predictions(str(tmp_path), "tless", "m", "r", is_refined=False)
    top1, multi = evaluate.read_estimates(paths[0]), evaluate.read_estimates(paths[1])
    n = sum(len(d["im_id"]) for d in batches)
    assert len(top1) == n and len(multi) == 3 * n
    d = batches[0]
    for h in range(3):
        e = multi[h]
        assert (e["scene_id"], e["im_id"], e["obj_id"]) == (2, int(d["im_id"][0]), int(d["object_id"][0]))
        assert np.float32(e["score"]) == d["scores"][0, h]
        np.testing.assert_array_equal(e["R"], d["poses"][0, h, :3, :3].astype(np.float64))     # the csv holds the f32's shortest repr
        np.testing.assert_array_equal(e["t"], d["poses"][0, h, :3, 3].astype(np.float64))
