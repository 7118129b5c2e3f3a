"""GPU: the four kernels behind the matcher's output -- topk_kernel / select_topk_kernel (gp_match.hip), ransac_kernel, recover_kernel,
rank_hypotheses_kernel (gp_pose.hip) -- against restatements of the reference's tensor formulation in float64
(gigapose_testing/pose_refs.py) and against the unmodified reference's outputs on the same inputs (tests/golden/pose_edges.npz), at
the layouts where they can go wrong: valid counts on both sides of every wave boundary and of the n = 46 switch between plain and fused
products, valid slots in chosen waves and lanes, first maxima among equal scores, weights that truncate, launch blocks of 63 / 64 / 65
(detection, hypothesis) pairs, payload pointers at chosen alignments, ties across the 64-lane stride.

RANSAC: M bit for bit one candidate's; the packed inlier list and the choice of the winner may differ from float64 only where an
error lies within c of the threshold (c = 2 x the error of a plain f32 evaluation, never taken from the kernel) -- on the built
problems nothing is that near, so 0 entries are excused; and bit for bit the reference's outputs, M included.  Recovery: rotation
entries, R^T R - I and |dt| / |t| within max(2 x the error of the reference's own f32 operator sequence against float64, a floor of a
few ulp; profiles/stage_tests_pose.txt).  Ranking and top-k: exact.  tests/test_pose_refs.py holds the CPU side: the preconditions and
the mutants each checker rejects.  Every test runs on both builds of the library (also_on_probe_binary)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import pose_refs as pr
from test_gpu_split import also_on_probe_binary, binary_name

pytestmark = pytest.mark.gpu
DEV = "cuda"


def t(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the cases are read-only arrays


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_edges.npz"))


# ----------------------------------------------------------------------------------------------------------------- RANSAC
def launch_ransac(L):
    """gp_ransac_scored on one launch's arrays, into buffers that carry one guard row past R -> numpy outputs (R rows)."""
    R = len(L["src_pts"])
    M = torch.full((R + 1, 3, 3), -7.0, device=DEV)
    failed = torch.full((R + 1,), 0xEE, dtype=torch.uint8, device=DEV)
    isrc = torch.full((R + 1, pr.P, 2), 12345, dtype=torch.int64, device=DEV)
    itar = torch.full((R + 1, pr.P, 2), 12345, dtype=torch.int64, device=DEV)
    isc = torch.full((R + 1, pr.P), 12345, dtype=torch.int64, device=DEV)
    w = None if L["weights"] is None else t(L["weights"])
    src, tar, scale, inplane = t(L["src_pts"]), t(L["tar_pts"]), t(L["rel_scale"]), t(L["rel_inplane"])      # held until the synchronisation below
    _lib.call("gp_ransac_scored", _lib.ptr(src), _lib.ptr(tar), _lib.ptr(scale), _lib.ptr(inplane),
              _lib.ptr(w), _lib.i(R), _lib.f(L["patch"]), _lib.f(L["thr"]), _lib.ptr(M), _lib.ptr(failed), _lib.ptr(isrc), _lib.ptr(itar),
              _lib.ptr(isc), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((M[R] == -7.0).all()) and int(failed[R]) == 0xEE, "the guard row past R was written"
    assert bool((isrc[R] == 12345).all()) and bool((itar[R] == 12345).all()) and bool((isc[R] == 12345).all()), "the guard row past R was written"
    f = failed[:R].cpu().numpy()
    assert set(np.unique(f)) <= {0, 1}
    return dict(M=M[:R].cpu().numpy(), failed=f.astype(bool), inl_src=isrc[:R].cpu().numpy(), inl_tar=itar[:R].cpu().numpy(),
                inl_score=isc[:R].cpu().numpy())


@also_on_probe_binary
@pytest.mark.parametrize("weights", pr.RANSAC_WEIGHTS)
@pytest.mark.parametrize("name", list(pr.RANSAC_LAUNCHES))
def test_ransac_vs_float64_and_reference(edges, name, weights):
    """Every edge problem of one (patch_size, pixel_threshold) in one launch: the float64 checker (nothing excused), and -- unit and
    dyadic weights -- the unmodified reference's five outputs bit for bit."""
    L = pr.ransac_launch(name, weights)
    out = launch_ransac(L)
    rep = pr.ransac_check(L, out)
    print(f"[{binary_name()}] {name} {weights}: {len(L['names'])} problems, checked {rep['checked']} excused {rep['excused']} failed {rep['failed']}; "
          f"largest c {max(rep['c'].values()):.3g}")
    assert rep["failed"] == 0, rep["first"]
    assert rep["excused"] <= pr.RANSAC_EXCUSED_CAP * rep["checked"] and rep["excused"] == 0
    if weights == "own":
        return
    tag = f"ransac_{name}_{weights}_"
    assert str(edges[tag + "inputs"]) == pr.ransac_launch_checksum(L), "the builders changed: regenerate pose_edges.npz"
    np.testing.assert_array_equal(out["M"].view(np.uint32), edges[tag + "M"].view(np.uint32))
    np.testing.assert_array_equal(out["failed"], edges[tag + "failed"])
    np.testing.assert_array_equal(out["inl_src"], edges[tag + "src_pts"].astype(np.int64))
    np.testing.assert_array_equal(out["inl_tar"], edges[tag + "tar_pts"].astype(np.int64))
    np.testing.assert_array_equal(out["inl_score"], edges[tag + "scores"].astype(np.int64))


@also_on_probe_binary
def test_ransac_permutation_and_unread_filler():
    """Permuting the problems permutes every output bit for bit; NaN instead of the -1000 filler of invalid slots changes nothing."""
    L = pr.ransac_launch("p14_t14")
    out = launch_ransac(L)
    perm = np.random.RandomState(3).permutation(len(L["names"]))
    outp = launch_ransac(pr.ransac_permuted(L, perm))
    outn = launch_ransac(pr.ransac_nan_filler(L))
    for k, v in out.items():
        v = v.view(np.uint32) if v.dtype == np.float32 else v
        np.testing.assert_array_equal(outp[k].view(v.dtype), v[perm], err_msg=k)
        np.testing.assert_array_equal(outn[k].view(v.dtype), v, err_msg=k)


# --------------------------------------------------------------------------------------------------------------- recovery
@also_on_probe_binary
@pytest.mark.parametrize("B,k", pr.RECOVERY_SHAPES)
def test_recovery_vs_float64_and_reference(edges, B, k):
    from gigapose_amd.poses import ObjectPoseRecovery

    c = pr.recovery_case(B, k)
    rec = ObjectPoseRecovery(t(c["tmpl_K"]), t(c["tmpl_M"]), t(c["tmpl_pose"]))
    args = (torch.from_numpy(c["labels0"].astype(np.int64) + 1), t(c["tar_K"]), t(c["tar_M"]), t(c["id_src"]), t(c["pred_M"]))
    _lib.status_word(DEV).zero_()
    poses = rec.forward_recovery(*args).cpu().numpy()
    assert _lib.take_status() == 0
    ref64, rot_b, trans_b, _ = pr.recovery_bounds(B, k)
    rot, orth, trans = pr.recovery_errors(poses, ref64)
    print(f"[{binary_name()}] (B, k) = ({B}, {k}): rotation {rot:.3g} / {rot_b:.3g}, R^T R - I {orth:.3g} / {rot_b:.3g}, |dt| / |t| {trans:.3g} / {trans_b:.3g}")
    assert pr.recovery_check(poses, B, k) is None, pr.recovery_check(poses, B, k)
    if B * k > 1:                                          # the reference itself raises at B = k = 1 (oracle/make_goldens.py)
        gold = edges[f"recovery_{B}_{k}_poses"]
        np.testing.assert_allclose(poses[..., :3, :3], gold[..., :3, :3], rtol=0, atol=2e-6)
        rel = np.linalg.norm(poses[..., :3, 3] - gold[..., :3, 3], axis=-1) / np.linalg.norm(gold[..., :3, 3], axis=-1)
        assert rel.max() < 1e-5
    # one crop transform that is no isotropic scale + translation, on the last detection (the last thread of the last block): raises
    for entry in ((0, 1), (1, 0), (1, 1)):
        bad = c["tar_M"].copy()
        bad[B - 1][entry] += 0.125
        with pytest.raises(AssertionError):
            rec.forward_recovery(args[0], args[1], t(bad), args[3], args[4])
    assert np.array_equal(rec.forward_recovery(*args).cpu().numpy().view(np.uint32), poses.view(np.uint32))      # the flag was cleared


# ---------------------------------------------------------------------------------------------------------------- ranking
def rank_collection(isc, payloads):
    import pandas as pd
    from gigapose_amd.tensor_collection import PandasTensorCollection

    return PandasTensorCollection(infos=pd.DataFrame(), ransac_scores=t(isc), **{n: t(v) for n, v in payloads.items()})


@also_on_probe_binary
@pytest.mark.parametrize("Pn", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_rank_vs_reference_arithmetic(k, Pn):
    """float32 sum / P (int64 -> f32, true division) and a stable descending sort: sums beyond 2^24 that round to one f32 are ties
    (lower index first), negative sums, all-equal rows."""
    from gigapose_amd.gigaPose import rank_hypotheses

    isc = pr.rank_scores_case(k, Pn)
    B = isc.shape[0]
    rs = np.random.RandomState(k + Pn)
    payloads = dict(M=rs.standard_normal((B, k, 3, 3)).astype(np.float32), flag=rs.uniform(size=(B, k)) < 0.5,
                    ids=rs.randint(0, 162, (B, k)).astype(np.int64))
    for sort in (True, False):
        score, order = pr.rank_restated(isc, sort)
        pred = rank_collection(isc, payloads)
        got = rank_hypotheses(pred, sort)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), order)
        np.testing.assert_array_equal(pred.scores.cpu().numpy().view(np.uint32), score.view(np.uint32))
        for n, v in dict(payloads, ransac_scores=isc).items():
            np.testing.assert_array_equal(getattr(pred, n).cpu().numpy(), np.take_along_axis(v, order.reshape(B, k, *[1] * (v.ndim - 2)), 1), err_msg=n)


@also_on_probe_binary
def test_rank_limits():
    from gigapose_amd.gigaPose import rank_hypotheses

    with pytest.raises(_lib.GigaPoseHipError):
        rank_hypotheses(rank_collection(np.ones((2, 65, 8), np.int64), {}))                   # k = GP_RANK_MAX_K + 1
    pred = rank_collection(np.zeros((0, 5, 256), np.int64), dict(M=np.zeros((0, 5, 3, 3), np.float32)))
    order = rank_hypotheses(pred)
    assert tuple(order.shape) == (0, 5) and tuple(pred.scores.shape) == (0, 5) and tuple(pred.M.shape) == (0, 5, 3, 3)


@also_on_probe_binary
@pytest.mark.parametrize("n_tensors", [16, 17, 33])
def test_rank_tensor_counts(n_tensors):
    """Exactly one launch's worth of tensors, one more, and two launches' worth plus one."""
    from gigapose_amd.gigaPose import rank_hypotheses

    isc = pr.rank_scores_case(5, 256)
    B, k = isc.shape[:2]
    rs = np.random.RandomState(n_tensors)
    payloads = {f"p{j:02d}": rs.standard_normal((B, k, 1 + j % 7)).astype(np.float32) for j in range(n_tensors - 1)}     # + ransac_scores
    pred = rank_collection(isc, payloads)
    assert len(pred.tensors) == n_tensors
    order = rank_hypotheses(pred).cpu().numpy()
    np.testing.assert_array_equal(order, pr.rank_restated(isc)[1])
    for n, v in payloads.items():
        np.testing.assert_array_equal(getattr(pred, n).cpu().numpy(), np.take_along_axis(v, order[:, :, None], 1), err_msg=n)


# (row bytes, source offset, destination offset) from a 512-byte-aligned address -> the copy route this must take
RANK_ROUTES = [(16, 0, 0, 16), (16, 4, 4, 4), (16, 1, 1, 1), (16, 0, 4, 4), (16, 4, 0, 4), (16, 8, 1, 1), (16, 2, 2, 1), (48, 16, 32, 16),
               (4, 0, 0, 4), (4, 1, 1, 1), (4, 3, 0, 1), (4, 8, 12, 4), (36, 0, 8, 4), (7, 0, 0, 1), (1, 5, 9, 1), (32, 12, 28, 4)]
GUARD = 64


@also_on_probe_binary
@pytest.mark.parametrize("k", [5, 64])
def test_rank_payload_copy_routes_by_pointer_alignment(k):
    """The 16-byte, 4-byte and 1-byte copy routes chosen by the ALIGNMENT of source and destination as well as by the row size: 16
    payloads at deliberately offset device addresses through the C ABI, a guard region around every destination."""
    isc = pr.rank_scores_case(k, 256)
    B = isc.shape[0]
    score, order = pr.rank_restated(isc)
    rs = np.random.RandomState(k)
    span = lambda rb: 512 * -(-(B * k * rb + 2 * GUARD + 64) // 512)
    total = sum(span(rb) for rb, _, _, _ in RANK_ROUTES)
    src_h = rs.randint(0, 256, total).astype(np.uint8)
    src_d, dst_d = t(src_h), torch.full((total,), 0xEE, dtype=torch.uint8, device=DEV)
    assert src_d.data_ptr() % 512 == 0 and dst_d.data_ptr() % 512 == 0
    at, srcs, dsts, rbs = 0, [], [], []
    for rb, so, do, route in RANK_ROUTES:
        s, d = at + GUARD + so, at + GUARD + do
        align = lambda p: 16 if p % 16 == 0 else 4 if p % 4 == 0 else 1
        assert min(align(rb), align(s), align(d)) == route and all(min(align(rb), align(s + b * k * rb), align(d + b * k * rb)) == route for b in range(B))
        srcs.append(s), dsts.append(d), rbs.append(rb)
        at += span(rb)
    n = len(RANK_ROUTES)
    scores_d, order_d, isc_d = torch.empty(B, k, device=DEV), torch.empty(B, k, dtype=torch.int64, device=DEV), t(isc)
    _lib.call("gp_rank_hypotheses", _lib.ptr(isc_d), _lib.i(B), _lib.i(k), _lib.i(256), _lib.i(1), _lib.ptr(scores_d), _lib.ptr(order_d), _lib.i(n),
              (ctypes.c_void_p * n)(*[src_d.data_ptr() + s for s in srcs]), (ctypes.c_void_p * n)(*[dst_d.data_ptr() + d for d in dsts]),
              (ctypes.c_int * n)(*rbs), _lib.stream_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(order_d.cpu().numpy(), order)
    np.testing.assert_array_equal(scores_d.cpu().numpy().view(np.uint32), score.view(np.uint32))
    want = np.full(total, 0xEE, np.uint8)
    for s, d, rb in zip(srcs, dsts, rbs):
        want[d:d + B * k * rb] = pr.rank_payload_expected(src_h[s:s + B * k * rb].reshape(B, k, rb), order).reshape(-1)
    np.testing.assert_array_equal(dst_d.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------------ top-k
@also_on_probe_binary
@pytest.mark.parametrize("N", pr.TOPK_N)
def test_topk_and_select_vs_lexsort_reference(N):
    """gp_topk and gp_select_topk, each against numpy lexsort on (-score, index) + take_along_axis + format_prediction restated: all-equal
    rows, ties across the 64-lane stride, negative rows, -0.0 against +0.0, the maximum at N - 1; k = 1, 5, N."""
    from gigapose_amd.matching import LocalSimilarity

    x = pr.topk_case(N)
    idx, sc, ma = pr.select_records_case(N)
    x_d, idx_d, sc_d, ma_d = t(x), t(idx), t(sc), t(ma)
    for k in sorted({1, min(5, N), N}):
        metric = LocalSimilarity(k=k, sim_threshold=0.5, patch_threshold=3)
        ids, scores, score_pts, tar_pts, src_pts = pr.select_restated(x, idx, sc, ma, k)
        got_ids, got_scores = metric.topk(x_d)
        np.testing.assert_array_equal(got_ids.cpu().numpy(), ids, err_msg=f"gp_topk k={k}")
        np.testing.assert_array_equal(got_scores.cpu().numpy().view(np.uint32), scores.view(np.uint32), err_msg=f"gp_topk k={k}")
        s_ids, s_scores, s_score_pts, s_tar, s_src = metric.select_topk(x_d, idx_d, sc_d, ma_d)
        np.testing.assert_array_equal(s_ids.cpu().numpy(), ids, err_msg=f"gp_select_topk k={k}")
        np.testing.assert_array_equal(s_scores.cpu().numpy().view(np.uint32), scores.view(np.uint32), err_msg=f"gp_select_topk k={k}")
        np.testing.assert_array_equal(s_score_pts.cpu().numpy().view(np.uint32), score_pts.view(np.uint32), err_msg=f"gp_select_topk k={k}")
        np.testing.assert_array_equal(s_tar.cpu().numpy(), tar_pts, err_msg=f"gp_select_topk k={k}")
        np.testing.assert_array_equal(s_src.cpu().numpy(), src_pts, err_msg=f"gp_select_topk k={k}")
        # the three stage kernels' point lists against the same restatement
        rec_idx, rec_score, rec_mask = metric.gather_records(got_ids, idx_d, sc_d, ma_d)
        g_tar, g_src = metric.format_points(rec_idx, rec_mask)
        np.testing.assert_array_equal(g_tar.cpu().numpy(), tar_pts, err_msg=f"gp_format_points k={k}")
        np.testing.assert_array_equal(g_src.cpu().numpy(), src_pts, err_msg=f"gp_format_points k={k}")
