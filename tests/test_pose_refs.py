"""CPU: the yardsticks of tests/test_gpu_pose_stages.py (gigapose_testing/pose_refs.py) -- the preconditions of the built cases, the
float64 restatements and the C oracle against the unmodified reference's outputs (tests/golden/pose_edges.npz), and the subtly wrong
implementations every checker rejects.  No GPU, no HIP library."""
import os

import numpy as np
import pytest
import torch

from gigapose_testing import pose_refs as pr
from gigapose_testing import synthetic as syn
from oracle import cpu as oracle

LAUNCHES = [(n, w) for n in pr.RANSAC_LAUNCHES for w in pr.RANSAC_WEIGHTS]


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_edges.npz"))


def golden_ransac(edges, name, w):
    tag = f"ransac_{name}_{w}_"
    L = pr.ransac_launch(name, w)
    assert str(edges[tag + "inputs"]) == pr.ransac_launch_checksum(L), "the builders changed: regenerate pose_edges.npz"
    return dict(M=edges[tag + "M"], failed=edges[tag + "failed"], inl_src=edges[tag + "src_pts"].astype(np.int64),
                inl_tar=edges[tag + "tar_pts"].astype(np.int64), inl_score=edges[tag + "scores"].astype(np.int64))


# ----------------------------------------------------------------------------------------------------------------- RANSAC
def test_ransac_problems_cover_the_listed_layouts():
    L = pr.ransac_launch("p14_t14")
    n = dict(zip(L["names"], (L["src_pts"][..., 0] != -1).sum(1)))
    assert [n[f"count_{c}"] for c in (0, 1, 2, 3, 45, 46, 63, 64, 65, 128, 255, 256)] == [0, 1, 2, 3, 45, 46, 63, 64, 65, 128, 255, 256]
    assert 40 <= len(L["names"]) <= 60 and all(len(pr.ransac_launch(s)["names"]) == 10 for s in ("p14_t5", "p16_t14", "p16_t5"))
    valid = lambda name: np.where(L["src_pts"][L["names"].index(name), :, 0] != -1)[0].tolist()
    assert valid("layout_slot0") == [0] and valid("layout_slot255") == [255] and valid("layout_wave3") == list(range(192, 256))
    assert valid("layout_waves03") == list(range(64)) + list(range(192, 256))
    assert valid("layout_lane0") == [0, 64, 128, 192] and valid("layout_lane63") == [63, 127, 191, 255]
    assert valid("layout_every2nd") == list(range(0, 256, 2))
    r = L["names"].index("src_y_minus_one")
    assert ((L["src_pts"][r, :, 0] != -1) & (L["src_pts"][r, :, 1] == -1)).sum() == 3
    r = L["names"].index("src_x_minus_one")
    assert ((L["src_pts"][r, :, 0] == -1) & (L["src_pts"][r, :, 1] != -1) & (L["rel_scale"][r] != pr.FILLER)).sum() == 5
    assert np.isnan(L["rel_scale"][L["names"].index("nan_scale")]).sum() == 1
    w = L["weights"]
    assert (w[L["names"].index("weights_zero")] == 0).all() and w[L["names"].index("weights_huge")].min() == 2.0 ** 24
    assert set(np.unique(pr.ransac_launch("p14_t14", "dyadic")["weights"])) == {-1.5, 0.0, 0.5, 1.0, 2.0, 2.75}


@pytest.mark.parametrize("name,w", LAUNCHES)
def test_ransac_restatement_is_accepted_with_nothing_excused(name, w):
    """The float64 restatement and its plain f32 evaluation both pass the checker; no decision of a built problem is excused, every
    unplanted error is RANSAC_MARGIN off the threshold (asserted by the builder) and c stays far below that margin."""
    L = pr.ransac_launch(name, w)
    for dtype in (np.float64, np.float32):
        rep = pr.ransac_check(L, pr.ransac_restated(L, dtype))
        assert rep["failed"] == 0, rep["first"]
        assert rep["excused"] == 0 and rep["checked"] > 100000
    assert max(rep["c"].values()) < pr.RANSAC_MARGIN / 2
    if name == "p14_t14":
        assert rep["c"]["exact_ties"] == 0.0 and rep["c"]["exact_ties_wave3"] == 0.0


def test_ransac_expected_decisions_of_the_planted_structure():
    L = pr.ransac_launch("p14_t14")
    out = pr.ransac_restated(L)
    tabs = {name: pr._tables(p) for name, p in zip(L["names"], pr._launch_problems(L))}
    length = dict(zip(L["names"], (out["inl_src"][..., 0] != -1).sum(1)))
    failed = dict(zip(L["names"], out["failed"]))

    def best(name):
        t = tabs[name]
        return int(np.where((t["M"].reshape(-1, 9) == out["M"][L["names"].index(name)].reshape(9)).all(1))[0][0])

    assert best("winner_first") == 0 and length["winner_first"] == 150
    assert best("winner_last_wave3") == 229 and length["winner_last_wave3"] == 180
    assert best("winner_mid_wave1") == 100 and length["winner_mid_wave1"] == 220
    assert best("weights_decide") == 14 and length["weights_decide"] == 9           # 9 x 2.75 beats 13 x 0.5: the later, smaller cluster
    assert best("two_clusters") == 0 and best("two_clusters_swapped") == 0 and length["two_clusters"] == 19      # the earlier cluster
    for name in ("no_consistent_pair", "no_consistent_pair_70", "count_1", "layout_slot0", "layout_slot255"):
        assert failed[name] and length[name] == 0 and best(name) == 0
    assert length["all_256_consistent"] == 255 and best("all_256_consistent") == 0
    assert failed["weights_zero"] and length["weights_zero"] > 20                   # failed with a non-empty inlier list
    assert not failed["nan_scale"] and length["nan_scale"] == 24                    # the NaN candidate is judged as a validation point
    assert length["exact_ties"] == 12                                               # the three exact-threshold members are inliers
    assert not failed["count_0"] and np.array_equal(out["M"][0], np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("mutant", pr.RANSAC_MUTANTS)
def test_ransac_checker_rejects_mutants(mutant):
    rejected = {w: pr.ransac_check(pr.ransac_launch("p14_t14", w), pr.ransac_restated(pr.ransac_launch("p14_t14", w), mutant=mutant))["failed"]
                for w in ("own", "dyadic")}
    print(mutant, "rejected on", rejected, "problems")
    assert rejected["own"] > 0 and rejected["dyadic"] > 0


@pytest.mark.parametrize("name,w", [(n, w) for n, w in LAUNCHES if w != "own"])
def test_ransac_oracle_and_restatement_vs_reference_golden(edges, name, w):
    """The unmodified reference's outputs on the edge problems: the C oracle equals them bit for bit (M included, n on both sides of
    torch's bmm switch at 46), and they pass the float64 checker."""
    L, g = pr.ransac_launch(name, w), golden_ransac(edges, name, w)
    rep = pr.ransac_check(L, g)
    assert rep["failed"] == 0 and rep["excused"] == 0, rep["first"]
    M, failed, isrc, itar, isc = oracle.ransac(L["src_pts"], L["tar_pts"], L["rel_scale"], L["rel_inplane"], float(L["patch"]), L["thr"], L["weights"])
    finite = np.isfinite(g["M"]).all((1, 2))
    assert finite.all()
    np.testing.assert_array_equal(M.view(np.uint32), g["M"].view(np.uint32))
    np.testing.assert_array_equal(failed, g["failed"])
    np.testing.assert_array_equal(isrc, g["inl_src"])
    np.testing.assert_array_equal(itar, g["inl_tar"])
    np.testing.assert_array_equal(isc, g["inl_score"])


def test_ransac_properties_of_the_restatement():
    L = pr.ransac_launch("p14_t14")
    out = pr.ransac_restated(L)
    perm = np.random.RandomState(3).permutation(len(L["names"]))
    outp = pr.ransac_restated(pr.ransac_permuted(L, perm))
    for k in out:
        np.testing.assert_array_equal(outp[k], out[k][perm])
    outn = pr.ransac_restated(pr.ransac_nan_filler(L))
    assert np.isnan(pr.ransac_nan_filler(L)["rel_scale"]).sum() > 2000
    for k in out:
        np.testing.assert_array_equal(outn[k], out[k])


# --------------------------------------------------------------------------------------------------------------- recovery
@pytest.mark.parametrize("B,k", pr.RECOVERY_SHAPES)
def test_recovery_restatement_oracle_and_golden(edges, B, k):
    case = pr.recovery_case(B, k)
    assert case["labels0"].min() == 0 or B == 1
    assert case["labels0"].max() == pr.RECOVERY_O - 1 and (case["id_src"].max() == pr.RECOVERY_N - 1 or B * k == 1)
    poses = case["tmpl_pose"].reshape(-1, 16)
    assert len(np.unique(poses, axis=0)) == len(poses)                               # a wrong gather shows
    s = case["tar_M"][:, 0, 0]
    assert s.min() >= 0.2 - 1e-6 and s.max() <= 4 + 1e-6 and (B == 1 or (s.min() < 0.21 and s.max() > 3.99))
    ref64, rot_b, trans_b, e32 = pr.recovery_bounds(B, k)
    print(f"(B, k) = ({B}, {k}): f32 evaluation / floor: rotation {e32[0] / pr.ROT_FLOOR:.3f} orthonormality {e32[1] / pr.ROT_FLOOR:.3f} "
          f"translation {e32[2] / pr.TRANS_FLOOR:.3f}")
    assert pr.recovery_check(pr.recover_restated(case, torch.float32), B, k) is None
    ours = oracle.recover(case["labels0"], case["tar_K"], case["tar_M"], case["id_src"], case["pred_M"], case["tmpl_K"], case["tmpl_M"], case["tmpl_pose"])
    assert pr.recovery_check(ours, B, k) is None, pr.recovery_check(ours, B, k)
    if B * k == 1:
        assert f"recovery_{B}_{k}_poses" not in edges.files         # the reference itself raises at this shape (oracle/make_goldens.py)
        return
    assert str(edges[f"recovery_{B}_{k}_inputs"]) == syn.checksum(*[case[n] for n in sorted(case)]), "the builders changed: regenerate pose_edges.npz"
    gold = edges[f"recovery_{B}_{k}_poses"]
    assert pr.recovery_check(gold, B, k) is None, pr.recovery_check(gold, B, k)
    np.testing.assert_allclose(ours[..., :3, :3], gold[..., :3, :3], rtol=0, atol=2e-6)     # the tolerances of the existing golden test
    rel = np.linalg.norm(ours[..., :3, 3] - gold[..., :3, 3], axis=-1) / np.linalg.norm(gold[..., :3, 3], axis=-1)
    assert rel.max() < 1e-5


@pytest.mark.parametrize("mutant", pr.RECOVERY_MUTANTS)
def test_recovery_checker_rejects_mutants(mutant):
    for B, k in pr.RECOVERY_SHAPES:
        for dtype in (torch.float32, torch.float64):
            assert pr.recovery_check(pr.recover_restated(pr.recovery_case(B, k), dtype, mutant), B, k) is not None, (B, k)


# ---------------------------------------------------------------------------------------------------------------- ranking
RANK_KP = [(k, Pn) for k in (1, 2, 63, 64) for Pn in (1, 255, 256, 257, 1000)]


def test_rank_cases_hold_f32_ties_of_different_integer_sums():
    for k, Pn in RANK_KP:
        if k == 1:
            continue
        isc = pr.rank_scores_case(k, Pn)
        s = isc.sum(2)
        assert s[2].min() >= 2 ** 25 and len(np.unique(s[2])) == min(k, 3)
        f = (torch.from_numpy(s[2].copy()) / Pn).numpy()
        assert f.dtype == np.float32 and (k < 3 or len(np.unique(f)) < 3)                     # different integers, the same f32
        assert s[3].max() <= 0 and s[3].min() < 0 and s[4].min() < 0 < s[4].max()
        score, order = pr.rank_restated(isc)
        assert (np.diff(score, axis=1) <= 0).all()
        tie = np.diff(score, axis=1) == 0
        assert tie.any() and (np.diff(order, axis=1)[tie] > 0).all()                          # a tie: the lower index first


@pytest.mark.parametrize("mutant", pr.RANK_MUTANTS)
def test_rank_mutants_differ(mutant):
    n = 0
    for k, Pn in RANK_KP:
        isc = pr.rank_scores_case(k, Pn)
        a, b = pr.rank_restated(isc), pr.rank_restated(isc, True, mutant)
        n += not (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]))
    assert n >= 12                                                                          # every shape with k > 1 (ties) / P > 1 (division)


# ------------------------------------------------------------------------------------------------------------------ top-k
def test_topk_restatement_vs_torch_where_torch_is_specified_and_the_oracle():
    for N in pr.TOPK_N:
        x = pr.topk_case(N)
        for k in sorted({1, min(5, N), N}):
            ids, sc = pr.topk_restated(x, k)
            tv, ti = torch.topk(torch.from_numpy(x.copy()), k, dim=1)
            np.testing.assert_array_equal(sc, tv.numpy())                                    # the values are specified, the tie order is not
            distinct = np.array([len(np.unique(r)) == N for r in x])
            np.testing.assert_array_equal(ids[distinct], ti.numpy()[distinct])
            oi, osc = oracle.topk(x, k)
            np.testing.assert_array_equal(oi, ids)
            np.testing.assert_array_equal(osc.view(np.uint32), sc.view(np.uint32))
        if N > 65:
            assert pr.topk_restated(x, 3)[0][2].tolist() == [63, 64, 127]                    # equal at n, n + 1, n + 64: by index
            assert pr.topk_restated(x, 1)[0][5, 0] == N - 1
            assert np.signbit(x[4]).any() and not np.signbit(x[4]).all()
            assert pr.topk_restated(x, 4)[0][4].tolist() == [i for i in range(6) if i != N // 2][:4]      # -0.0 == +0.0: by index


@pytest.mark.parametrize("mutant", pr.TOPK_MUTANTS)
def test_topk_mutants_differ(mutant):
    n = 0
    for N in pr.TOPK_N[1:]:
        x = pr.topk_case(N)
        a, b = pr.topk_restated(x, min(5, N)), pr.topk_restated(x, min(5, N), mutant)
        n += not np.array_equal(a[0], b[0])
    assert n == len(pr.TOPK_N) - 1


def test_select_restatement_vs_oracle_gather_format():
    N, k = 65, 5
    x = pr.topk_case(N)
    idx, sc, ma = pr.select_records_case(N)
    ids, scores, score_pts, tar_pts, src_pts = pr.select_restated(x, idx, sc, ma, k)
    o_sp, o_tar, o_src = oracle.gather_format(ids, idx, sc, ma)
    np.testing.assert_array_equal(score_pts.view(np.uint32), o_sp.view(np.uint32))
    np.testing.assert_array_equal(tar_pts, o_tar)
    np.testing.assert_array_equal(src_pts, o_src)
    assert ((tar_pts[..., 0] == -1) == (src_pts[..., 0] == -1)).all() and 0.2 < (tar_pts[..., 0] == -1).mean() < 0.4
