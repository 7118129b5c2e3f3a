"""Float64 restatements, edge-case builders, checkers and mutants for the four kernels behind the matcher's output:
topk_kernel / select_topk_kernel (gp_match.hip) and ransac_kernel, recover_kernel, rank_hypotheses_kernel (gp_pose.hip).

The restatements follow the reference's TENSOR formulation (ransac.py:19-172, poses.py:26-122, lib3d/torch.py, gigaPose.py:588-594,
matching.py:279-316): an (n, n-1) validation-index table, gathers, one batched 3x3 product over the validation points, `max` taking
the first maximum, `where` for the inlier list, the packed write-back, torch.inverse for query_K, gather along the view axis.  They
are written from those files, not from gp_pose.hip or oracle/gp_oracle.c (whose loops are twins of the kernels), so a misreading
the two twins share does not pass here.  tests/test_pose_refs.py holds the CPU side (preconditions of the cases, the mutants every
checker rejects), tests/test_gpu_pose_stages.py the kernels.

RANSAC's rule (match_tiles_check of stage_refs.py is the model): the candidates' M is plain f32 mul / add and therefore compared
bit for bit; every error e[i, j] is evaluated in float64, and a decision `e <= threshold` may differ only where |e - threshold| < c,
c = 2 x the largest difference between a plain f32 evaluation of the same errors and float64 over the problem.  Such entries are
counted, and at most RANSAC_EXCUSED_CAP of a problem's decisions may be excused.  The builders assert at build time that no error
they did not plant sits within RANSAC_MARGIN px of the threshold, so on the built problems nothing is excused.  Errors of exactly
the threshold up to rounding (synthetic.many_to_one_case) stay with the reference goldens; the ties planted here are exact in
every precision (a pure translation of points on one grid row: every error is an integer, c = 0).  Weights of the 2^24 class are
2^24 and 2^33: sums of up to 255 of them are exact in f32 in any order, and 2^33 does not survive a truncation through int32.

NaN scores are out of scope of the top-k reference: the range guards in front of the matcher stop them upstream."""
import functools

import numpy as np
import torch

from .synthetic import checksum

P = 256
G = 16
FILLER = -1000.0                 # what the pipeline leaves in the scale / in-plane slots of an invalid correspondence
RANSAC_MARGIN = 1e-3             # px: no unplanted error of a built problem is nearer to the threshold
RANSAC_EXCUSED_CAP = 0.005       # the matcher's MATCH_EXCUSED_CAP: a condition, not a measurement
RANSAC_NOISE = 3e-3              # relative scale / angle noise of a consistent correspondence: <= ~2.5 px over the 224 px crop


# ================================================================================================================= RANSAC
def _slots(kind, n, rs):
    if kind == "random":
        return np.sort(rs.choice(P, n, replace=False))
    return np.asarray({"slot0": [0], "slot255": [255], "wave3": range(192, 256), "waves03": list(range(64)) + list(range(192, 256)),
                       "lane0": [0, 64, 128, 192], "lane63": [63, 127, 191, 255], "every2nd": range(0, 256, 2), "every2nd_odd": range(1, 256, 2),
                       "all": range(256)}[kind])


_DISPLACEMENTS = [(3 * a, 3 * b) for a in range(-6, 7) for b in range(-6, 7) if (a, b) != (0, 0)]      # patches: >= 42 px apart


def _problem(seed, slots, roles, turns=0, scale=1.0, angle=None, noise=RANSAC_NOISE, weights=None, patch=14, thr=14.0, nan_at=None,
             y_minus_one=(), x_minus_one=(), tie_at=(), one_row=False):
    """One problem of 256 slots.  roles (per valid correspondence, in slot order): 0 / 1 = consistent with cluster 0 / 1 (their
    translations lie 40 patches apart), -1 = on cluster 0's positions but with its rotation turned by 180 degrees (a candidate that
    finds nobody, a validation point like any other), -2 = an outlier, displaced from cluster 0 by a vector of its own.
    angle None: a lattice similarity (quarter `turns`, integer scale) that maps the grid onto integers; else a general one, whose
    rounded targets put errors anywhere around the threshold -- the seed is advanced until RANSAC_MARGIN holds."""
    slots, roles = np.asarray(slots), np.asarray(roles)
    n = len(slots)
    for attempt in range(200):
        rs = np.random.RandomState(seed + 7919 * attempt)
        grid = np.stack([np.arange(P) % G, np.arange(P) // G], 1)[rs.permutation(P)]
        src = grid[:n].astype(np.int64)
        if one_row:                                                                          # all on one grid row, displaced along x only:
            src = np.stack([rs.permutation(G)[:n], np.full(n, 3)], 1).astype(np.int64)       # every error is an integer, exact in f32
        for j in y_minus_one:
            src[j, 1] = -1
        th = turns * np.pi / 2 if angle is None else angle
        c, s = (np.round(np.cos(th)), np.round(np.sin(th))) if angle is None else (np.cos(th), np.sin(th))
        S = scale * np.array([[c, -s], [s, c]])
        t0 = rs.randint(-6, 7, 2).astype(np.float64)
        disp = np.zeros((n, 2))
        disp[roles == 1] = (40, -40)
        out = np.where(roles == -2)[0]
        disp[out] = np.asarray(_DISPLACEMENTS)[rs.permutation(len(_DISPLACEMENTS))[:len(out)]]
        if one_row:
            disp[out] = np.stack([3 * (1 + np.arange(len(out))) * np.where(np.arange(len(out)) % 2, -1, 1), np.zeros(len(out))], 1)
        for j in tie_at:
            disp[j] = (thr / patch, 0)                                                   # exactly the threshold, along x
        tar = np.round(src @ S.T + t0 + disp).astype(np.int64)
        ang = th + noise * rs.uniform(-1, 1, n) + np.pi * (roles == -1)
        sc = scale * (1 + noise * rs.uniform(-1, 1, n))
        prob = dict(src=np.full((P, 2), -1, np.int64), tar=np.full((P, 2), -1, np.int64), scale=np.full(P, FILLER, np.float32),
                    inplane=np.full((P, 2), FILLER, np.float32), weight=np.ones(P, np.float32), patch=patch, thr=float(thr))
        prob["src"][slots], prob["tar"][slots] = src, tar
        prob["scale"][slots] = sc
        cs_sn = np.stack([np.cos(ang), np.sin(ang)], 1)
        prob["inplane"][slots] = cs_sn if noise or angle is not None else np.round(cs_sn)    # no noise on a lattice: exactly 0 / 1 / -1
        if nan_at is not None:
            prob["scale"][slots[nan_at]] = np.nan
        free = np.setdiff1d(np.arange(P), slots)
        for j, f in zip(x_minus_one, free):                                              # x = -1, everything else live: still invalid
            prob["src"][f] = (-1, 5)
            prob["tar"][f] = tar[j]
            prob["scale"][f], prob["inplane"][f] = prob["scale"][slots[j]], prob["inplane"][slots[j]]
        if weights is not None:
            prob["weight"] = np.asarray(weights(rs), np.float32)
        tab = _tables(prob)
        if n < 2:
            return prob
        e = tab["e64"][~np.eye(n, dtype=bool)]
        near = np.abs(e - thr) < RANSAC_MARGIN
        planted = 2 * len(tie_at) * (int((roles == 0).sum()) - len(tie_at))     # a displaced member and a member in place, either way round
        if near.sum() == planted and (planted == 0 or tab["c"] == 0.0):
            return prob
    raise AssertionError("no seed keeps every unplanted error %g px off the threshold" % RANSAC_MARGIN)


def _dyadic(rs):
    return rs.choice(np.array([0.5, 2.75, -1.5, 1.0, 2.0, 0.0], np.float32), P)


def _huge(rs):
    return rs.choice(np.array([2.0 ** 24, 2.0 ** 33], np.float32), P)      # sums of <= 255 of these are exact in f32 in any order


def _mixed(rs, n, share_out=0.25):
    r = np.zeros(n, int)
    r[rs.permutation(n)[:int(n * share_out)]] = -2
    return r


def ransac_problems(patch=14, thr=14.0):
    """name -> problem, for one launch at (patch_size, pixel_threshold)."""
    rs = np.random.RandomState(31)
    kw = dict(patch=patch, thr=thr)
    out = {}
    for i, n in enumerate((0, 1, 2, 3, 45, 46, 63, 64, 65, 128, 255, 256)):                # valid counts, random slots
        general = 2 <= n <= 65                                                              # general similarity: errors all over the range
        out[f"count_{n}"] = _problem(100 + i, _slots("random", n, rs), _mixed(rs, n), turns=i % 4, scale=0.8 + 0.05 * i if general else 1.0 + (i % 2),
                                     angle=0.3 + 0.4 * i if general else None, **kw)
    for i, kind in enumerate(("slot0", "slot255", "wave3", "waves03", "lane0", "lane63", "every2nd", "every2nd_odd")):
        sl = _slots(kind, 0, rs)
        out[f"layout_{kind}"] = _problem(200 + i, sl, _mixed(rs, len(sl)), turns=i % 4, **kw)
    # one hub whose similarity everybody's POSITION agrees with; the others' own rotation is turned: a unique winner
    sl = _slots("random", 200, rs)
    out["winner_first"] = _problem(301, sl, [0] + [-1] * 150 + [-2] * 49, turns=1, **kw)
    sl = _slots("all", 0, rs)[:230]
    out["winner_last_wave3"] = _problem(302, sl, [-1] * 180 + [-2] * 49 + [0], turns=3, **kw)
    # two disjoint clusters of 20 with the same score: cluster 1 starts in wave 0, cluster 0 in wave 2; the earlier one (cluster 1) wins
    sl = np.concatenate([np.arange(5, 25), np.arange(130, 150), np.arange(200, 210)])
    out["two_clusters"] = _problem(303, sl, [1] * 20 + [0] * 20 + [-2] * 10, turns=2, **kw)
    sl = np.concatenate([np.arange(40, 60), np.arange(100, 110), np.arange(230, 250)])
    out["two_clusters_swapped"] = _problem(304, sl, [0] * 20 + [-2] * 10 + [1] * 20, **kw)
    out["no_consistent_pair"] = _problem(305, _slots("random", 7, rs), [-2] * 7, turns=1, **kw)
    out["no_consistent_pair_70"] = _problem(306, _slots("random", 70, rs), [-2] * 70, **kw)
    out["all_256_consistent"] = _problem(307, _slots("all", 0, rs), [0] * 256, turns=1, **kw)
    out["src_y_minus_one"] = _problem(308, _slots("random", 40, rs), _mixed(rs, 40), y_minus_one=(0, 7, 39), **kw)
    out["src_x_minus_one"] = _problem(309, _slots("random", 40, rs), _mixed(rs, 40), x_minus_one=(1, 2, 3, 4, 5), turns=2, **kw)
    out["weights_zero"] = _problem(310, _slots("random", 50, rs), _mixed(rs, 50), weights=lambda r: np.zeros(P), **kw)
    out["weights_dyadic"] = _problem(311, _slots("random", 90, rs), _mixed(rs, 90), weights=_dyadic, turns=3, **kw)
    out["weights_dyadic_clusters"] = _problem(312, np.arange(20, 80), [0] * 25 + [1] * 30 + [-2] * 5, weights=_dyadic, **kw)
    out["weights_huge"] = _problem(313, _slots("random", 120, rs), _mixed(rs, 120), weights=_huge, turns=1, **kw)
    # 10 members of weight 2.75 (slots 100..109) against 14 of weight 0.5 (slots 20..33): the smaller, later cluster wins by weight
    by_cluster = lambda r: np.where((np.arange(P) >= 100) & (np.arange(P) < 110), 2.75, 0.5)
    out["weights_decide"] = _problem(318, np.concatenate([np.arange(20, 34), np.arange(100, 110)]), [1] * 14 + [0] * 10, weights=by_cluster, **kw)
    out["winner_mid_wave1"] = _problem(319, _slots("all", 0, rs), [-1] * 100 + [0] + [-1] * 120 + [-2] * 35, turns=2, **kw)
    out["layout_wave_edges"] = _problem(320, [63, 64, 127, 128, 191, 192], [0, 0, -2, 0, 0, 0], turns=3, **kw)
    out["layout_wave3_empty"] = _problem(321, np.arange(192), _mixed(rs, 192), scale=2.0, **kw)
    out["nan_scale"] = _problem(314, _slots("random", 30, rs), [0] * 25 + [-2] * 5, nan_at=9, **kw)
    out["nan_scale_wave_edge"] = _problem(315, _slots("waves03", 0, rs), _mixed(rs, 128), nan_at=64, turns=2, **kw)
    # every quantity exact in f32 and float64 (no noise, a translation, all points on one row: integer errors): an error of EXACTLY the
    # threshold is an inlier in every precision, c = 0, and nothing is excused
    if thr % patch == 0:
        out["exact_ties"] = _problem(316, _slots("random", 16, rs), [0] * 13 + [-2] * 3, noise=0.0, tie_at=(3, 7, 12), one_row=True, **kw)
        out["exact_ties_wave3"] = _problem(317, np.arange(236, 252), [-2, -2] + [0] * 14, noise=0.0, tie_at=(2, 15), one_row=True, turns=2, **kw)
    return out


RANSAC_LAUNCHES = {"p14_t14": (14, 14.0), "p14_t5": (14, 5.0), "p16_t14": (16, 14.0), "p16_t5": (16, 5.0)}
RANSAC_WEIGHTS = ("unit", "own", "dyadic")      # ones (a null pointer); each problem's own weights; dyadic fractions on every problem


@functools.lru_cache(maxsize=None)
def ransac_launch(name, weights="own"):
    """All problems of one (patch_size, pixel_threshold) as the arrays of one launch; the side launches keep a sub-set."""
    patch, thr = RANSAC_LAUNCHES[name]
    probs = ransac_problems(patch, thr)
    if name != "p14_t14":
        keep = ("count_0", "count_1", "count_45", "count_46", "count_65", "count_256", "layout_waves03", "winner_last_wave3", "two_clusters",
                "weights_dyadic")
        probs = {k: probs[k] for k in keep}
    names = list(probs)
    st = lambda key: np.stack([probs[n][key] for n in names])
    L = dict(name=name, names=names, src_pts=st("src"), tar_pts=st("tar"), rel_scale=st("scale"), rel_inplane=st("inplane"), patch=patch, thr=thr,
             weights=None if weights == "unit" else st("weight"))
    if weights == "dyadic":
        L["weights"] = np.stack([_dyadic(np.random.RandomState(900 + i)) for i in range(len(names))])
    for v in L.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return L


def ransac_launch_checksum(L):
    w = L["weights"] if L["weights"] is not None else np.zeros(0, np.float32)
    return checksum(L["src_pts"], L["tar_pts"], np.nan_to_num(L["rel_scale"], nan=-7.0), L["rel_inplane"], w)


def _val_idx(n):
    """RANSAC._sample's remaining_idx: row i = 0..n-1 without i  (n, n-1)."""
    col = np.arange(n - 1)[None, :]
    return col + (col >= np.arange(n)[:, None])


def _candidates_f32(src, tar, sc, cs, sn, patch, centre=False):
    """M of every candidate in numpy f32, plain mul / add in the reference's order (affine_torch; apply_affine on the one
    training point with a zero translation column; M[:, :2, 2] = tar - that): bit-reproducible."""
    f = np.float32
    x, y = (src * patch).astype(f).T
    u, v = (tar * patch).astype(f).T
    if centre:
        x, y, u, v = (a + f(patch / 2) for a in (x, y, u, v))
    M = np.zeros((len(sc), 3, 3), f)
    M[:, 2, 2] = 1
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = cs * sc, (-sn) * sc, sn * sc, cs * sc
    with np.errstate(invalid="ignore"):
        a0 = (M[:, 0, 0] * x + M[:, 0, 1] * y) + f(0) * f(1)
        a1 = (M[:, 1, 0] * x + M[:, 1, 1] * y) + f(0) * f(1)
    M[:, 0, 2], M[:, 1, 2] = u - a0, v - a1
    return M, np.stack([x, y], 1), np.stack([u, v], 1)


def _errors(M, sp, tp, val_idx, dtype):
    """errors[i, j'] = | tar[val_idx[i, j']] - M_i src[val_idx[i, j']] | : gathers, one batched 3x3 product, a norm -- in `dtype`."""
    Mh, vs, vt = M.astype(dtype), sp.astype(dtype)[val_idx], tp.astype(dtype)[val_idx]          # (n,3,3) (n,m,2) (n,m,2)
    with np.errstate(invalid="ignore"):
        a0 = (Mh[:, None, 0, 0] * vs[..., 0] + Mh[:, None, 0, 1] * vs[..., 1]) + Mh[:, None, 0, 2]
        a1 = (Mh[:, None, 1, 0] * vs[..., 0] + Mh[:, None, 1, 1] * vs[..., 1]) + Mh[:, None, 1, 2]
        d0, d1 = vt[..., 0] - a0, vt[..., 1] - a1
        return np.sqrt(d0 * d0 + d1 * d1)


def _compact(prob, from_y=False):
    mask = prob["src"][:, 1 if from_y else 0] != -1                                            # mask = src_keypoint[:, 0] != -1
    return mask, prob["src"][mask], prob["tar"][mask], prob["scale"][mask], prob["inplane"][mask, 0], prob["inplane"][mask, 1], prob["weight"][mask]


def _tables(prob):
    """What the checker holds a problem to: the candidates' f32 M, the (n, n) float64 errors (inf on the diagonal) and c."""
    mask, src, tar, sc, cs, sn, w = _compact(prob)
    n = int(mask.sum())
    tab = dict(n=n, thr=prob["thr"], src=src, tar=tar, w=w, c=0.0)
    if n == 0:
        return tab
    M, sp, tp = _candidates_f32(src, tar, sc, cs, sn, prob["patch"])
    full = np.broadcast_to(np.arange(n), (n, n))
    e64, e32 = _errors(M, sp, tp, full, np.float64), _errors(M, sp, tp, full, np.float32)
    off = ~np.eye(n, dtype=bool) & np.isfinite(e64)
    tab.update(M=M, c=2.0 * float(np.abs(e32.astype(np.float64) - e64)[off].max()) if off.any() else 0.0)
    e64[np.eye(n, dtype=bool)] = np.inf
    tab["e64"] = e64
    return tab


def _launch_problems(L):
    w = L["weights"] if L["weights"] is not None else np.ones(L["rel_scale"].shape, np.float32)
    return [dict(src=L["src_pts"][r], tar=L["tar_pts"][r], scale=L["rel_scale"][r], inplane=L["rel_inplane"][r], weight=w[r], patch=L["patch"],
                 thr=L["thr"]) for r in range(len(L["src_pts"]))]


RANSAC_MUTANTS = ("counts_itself", "last_maximum", "valid_from_y", "strict_less", "patch_centre", "weights_rounded", "unpacked")


def ransac_restated(L, dtype=np.float64, mutant=None):
    """RANSAC.forward on one launch, errors in `dtype`; `mutant` = one subtly wrong reading of it.  -> the kernel's five outputs."""
    R = len(L["src_pts"])
    out = dict(M=np.broadcast_to(np.eye(3, dtype=np.float32), (R, 3, 3)).copy(), failed=np.zeros(R, bool), inl_src=np.full((R, P, 2), -1, np.int64),
               inl_tar=np.full((R, P, 2), -1, np.int64), inl_score=np.zeros((R, P), np.int64))
    for r, prob in enumerate(_launch_problems(L)):
        mask, src, tar, sc, cs, sn, w = _compact(prob, from_y=mutant == "valid_from_y")
        n = int(mask.sum())
        if n == 0:
            continue
        M, sp, tp = _candidates_f32(src, tar, sc, cs, sn, prob["patch"], centre=mutant == "patch_centre")
        val_idx = np.broadcast_to(np.arange(n), (n, n)) if mutant == "counts_itself" else _val_idx(n)
        err = _errors(M, sp, tp, val_idx, dtype)
        with np.errstate(invalid="ignore"):
            inliers = err < prob["thr"] if mutant == "strict_less" else err <= prob["thr"]
        score = (inliers * w.astype(np.float64)[val_idx]).sum(1)
        best = int(np.argmax(score)) if mutant != "last_maximum" else n - 1 - int(np.argmax(score[::-1]))     # max: the first maximum
        out["M"][r] = M[best]
        out["failed"][r] = score[best] == 0
        idx = val_idx[best][np.where(inliers[best])[0]]
        wi = (np.rint(w[idx]) if mutant == "weights_rounded" else np.trunc(w[idx])).astype(np.int64)            # assignment into an int64 tensor
        at = np.where(mask)[0][idx] if mutant == "unpacked" else np.arange(len(idx))
        out["inl_src"][r, at], out["inl_tar"][r, at], out["inl_score"][r, at] = src[idx], tar[idx], wi
    return out


def _check_problem(tab, M, failed, isrc, itar, isc):
    """None, or what is wrong with the kernel's answer to one problem."""
    n, thr, c = tab["n"], tab["thr"], tab["c"]
    pad = lambda q: (isrc[q:] == -1).all() and (itar[q:] == -1).all() and (isc[q:] == 0).all()
    if n == 0:
        ok = np.array_equal(M.view(np.uint32), np.eye(3, dtype=np.float32).view(np.uint32)) and not failed and pad(0)
        return None if ok else "n = 0: identity M, not failed and an empty list expected"
    same = (tab["M"].view(np.uint32).reshape(n, 9) == M.view(np.uint32).reshape(9)).all(1)
    if not same.any():
        return "M is no candidate's M bit for bit"
    e, w = tab["e64"], tab["w"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        near = np.abs(e - thr) < c
        sure = (e <= thr) & ~near
    lo = (sure * w).sum(1) + (near * np.minimum(w, 0)).sum(1)
    hi = (sure * w).sum(1) + (near * np.maximum(w, 0)).sum(1)
    wt = np.trunc(tab["w"]).astype(np.int64)
    why = None
    for best in np.where(same)[0]:
        q, why = 0, None
        for j in range(n):
            hit = q < P and (isrc[q] == tab["src"][j]).all() and (itar[q] == tab["tar"][j]).all() and isc[q] == wt[j]
            if sure[best, j] and not hit:
                why = f"candidate {best}: certain inlier {j} (error {e[best, j]:.6f}) is not entry {q} of the packed list"
                break
            q += int(bool(hit and (sure[best, j] or near[best, j])))
        if why is None and not pad(q):
            why = f"candidate {best}: the list goes on behind its {q} inliers, or its padding is not -1 / 0"
        if why is None and ((lo[:best] >= hi[best]).any() or (lo[best + 1:] > hi[best]).any()):
            why = f"candidate {best} (score <= {hi[best]}) is not the first maximum: scores {lo[:best + 1].max()} before / {lo[best:].max()} from it on"
        if why is None and lo[best] == hi[best] and bool(failed) != (lo[best] == 0):
            why = f"failed = {bool(failed)} at score {lo[best]}"
        if why is None and not (lo[best] <= 0 <= hi[best]) and failed:
            why = "failed at a score that cannot be 0"
        if why is None:
            return None
    return why


def ransac_check(L, out):
    """-> dict(checked, excused, failed, first, per problem c and excused counts)."""
    rep = dict(checked=0, excused=0, failed=0, first=None, c={}, excused_by={})
    for r, (name, prob) in enumerate(zip(L["names"], _launch_problems(L))):
        tab = _tables(prob)
        n = tab["n"]
        ex = 0
        if n >= 2:
            with np.errstate(invalid="ignore"):
                ex = int((np.abs(tab["e64"] - tab["thr"]) < tab["c"]).sum())
        rep["checked"] += n * (n - 1)
        rep["excused"] += ex
        rep["c"][name], rep["excused_by"][name] = tab["c"], ex
        why = _check_problem(tab, out["M"][r], out["failed"][r], out["inl_src"][r], out["inl_tar"][r], out["inl_score"][r])
        if why is None and ex > RANSAC_EXCUSED_CAP * max(n * (n - 1), 1):
            why = f"{ex} of {n * (n - 1)} decisions excused"
        if why is not None:
            rep["failed"] += 1
            rep["first"] = rep["first"] or f"{name} (problem {r}, n = {n}): {why}"
    return rep


def ransac_permuted(L, perm):
    return {k: (v[perm] if isinstance(v, np.ndarray) else ([v[i] for i in perm] if k == "names" else v)) for k, v in L.items()}


def ransac_nan_filler(L):
    """The same launch with NaN where the invalid slots hold -1000: they are never read."""
    M = dict(L)
    inv = L["src_pts"][..., 0] == -1
    M["rel_scale"], M["rel_inplane"] = L["rel_scale"].copy(), L["rel_inplane"].copy()
    M["rel_scale"][inv & (L["rel_scale"] == FILLER)] = np.nan
    M["rel_inplane"][(inv[..., None] & (L["rel_inplane"] == FILLER))] = np.nan
    return M


# =============================================================================================================== recovery
RECOVERY_SHAPES = ((1, 1), (63, 1), (13, 5), (64, 1), (65, 1), (26, 5), (10, 13))     # (B, k): B k = 1, 63, 65, 64, 65, 130, 130
RECOVERY_O, RECOVERY_N = 3, 7
ROT_FLOOR = 8 * 2.0 ** -24       # a rotation entry: a division by a norm and a 3-term dot product of values <= 1
TRANS_FLOOR = 32 * 2.0 ** -24    # |dt| / |t|: five 3-term products over pixel coordinates of ~1e3 against offsets from the principal point
RECOVERY_MUTANTS = ("rotation_order", "scale_from_pred_M", "focal_ratio_inverted", "crop_not_inverted")


def _rotation(rs):
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def recovery_case(B, k):
    rs = np.random.RandomState(1000 * B + k)
    O, N = RECOVERY_O, RECOVERY_N
    tK = np.zeros((O, 3, 3), np.float32)
    tK[:, 0, 0], tK[:, 1, 1], tK[:, 0, 2], tK[:, 1, 2], tK[:, 2, 2] = rs.uniform(500, 700, O), rs.uniform(500, 700, O), 320, 240, 1
    tM = np.zeros((O, N, 3, 3), np.float32)
    tM[..., 0, 0] = tM[..., 1, 1] = rs.uniform(0.8, 2.5, (O, N))
    tM[..., 0, 2], tM[..., 1, 2], tM[..., 2, 2] = rs.uniform(-400, -50, (O, N)), rs.uniform(-300, -20, (O, N)), 1
    tP = np.zeros((O, N, 4, 4), np.float32)
    for o in range(O):
        for v in range(N):                                                                   # every (label, view) its own pose
            tP[o, v, :3, :3] = _rotation(rs)
            tP[o, v, :3, 3] = (rs.uniform(-20, 20), rs.uniform(-20, 20), 350 + 10 * (o * N + v))
            tP[o, v, 3] = (0, 0, 0, 1)
    tP[0, 0, 3] = (0.25, -0.5, 3.0, 1.0)                                                      # row 3 is copied, whatever it holds
    qK = np.zeros((B, 3, 3), np.float32)
    f = rs.uniform(500, 1200, B)
    qK[:, 0, 0], qK[:, 1, 1], qK[:, 0, 2], qK[:, 1, 2], qK[:, 2, 2] = f, f * rs.uniform(0.98, 1.02, B), rs.uniform(280, 360, B), rs.uniform(200, 280, B), 1
    qM = np.zeros((B, 3, 3), np.float32)
    s = np.exp(rs.uniform(np.log(0.2), np.log(4.0), B))
    s[0], s[-1] = 0.2, 4.0
    qM[:, 0, 0] = qM[:, 1, 1] = s
    qM[:, 0, 2], qM[:, 1, 2], qM[:, 2, 2] = rs.uniform(-300, 50, B) * s, rs.uniform(-300, 50, B) * s, 1
    labels0 = rs.randint(0, O, B).astype(np.int32)
    id_src = rs.randint(0, N, (B, k)).astype(np.int64)
    labels0[0], labels0[-1] = (0, O - 1) if B > 1 else (O - 1, O - 1)
    id_src[0, 0], id_src[-1, -1] = (0, N - 1) if B * k > 1 else (N - 1, N - 1)
    id_src[B // 2, k // 2] = 0
    ms, ma = rs.uniform(0.3, 2.0, (B, k)), rs.uniform(-np.pi, np.pi, (B, k))
    pM = np.zeros((B, k, 3, 3), np.float32)
    pM[..., 0, 0], pM[..., 0, 1], pM[..., 1, 0], pM[..., 1, 1] = ms * np.cos(ma), -ms * np.sin(ma), ms * np.sin(ma), ms * np.cos(ma)
    pM[..., 0, 2], pM[..., 1, 2], pM[..., 2, 2] = rs.uniform(-100, 100, (B, k)), rs.uniform(-100, 100, (B, k)), 1
    pM[rs.uniform(size=(B, k)) < 0.15] = np.eye(3, dtype=np.float32)                          # RANSAC's answer to n = 0
    if B * k > 1:
        pM[-1, -1] = np.eye(3, dtype=np.float32)
    case = dict(labels0=labels0, tar_K=qK, tar_M=qM, id_src=id_src, pred_M=pM, tmpl_K=tK, tmpl_M=tM, tmpl_pose=tP)
    for v in case.values():
        v.setflags(write=False)
    return case


def recover_restated(case, dtype=torch.float64, mutant=None):
    """ObjectPoseRecovery.forward_recovery with the reference's operator sequence, in `dtype` (float64: the yardstick; float32: the
    reference's own arithmetic, whose error against float64 sizes the bound)."""
    T = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    lab = torch.from_numpy(np.array(case["labels0"])).long()
    ids = torch.from_numpy(np.array(case["id_src"])).long()
    tP, tM, tK = T(case["tmpl_pose"])[lab], T(case["tmpl_M"])[lab], T(case["tmpl_K"])[lab]
    qM, qK, pM = T(case["tar_M"]), T(case["tar_K"]), T(case["pred_M"])
    B, k = ids.shape
    temp_Ks = tK[:, None].expand(B, k, 3, 3)
    temp_Ms = torch.gather(tM, 1, ids[:, :, None, None].expand(B, k, 3, 3))
    poses = torch.gather(tP, 1, ids[:, :, None, None].expand(B, k, 4, 4)).clone()
    Rin = torch.zeros_like(pM)
    Rin[:, :, 2, 2] = 1
    Rin[:, :, :2, :2] = pM[:, :, :2, :2] / torch.norm(pM[:, :, :2, 0], dim=2)[:, :, None, None]
    Rt = poses[:, :, :3, :3].clone()
    poses[:, :, :3, :3] = torch.matmul(Rt, Rin) if mutant == "rotation_order" else torch.matmul(Rin, Rt)
    temp_z = poses[:, :, 2, 3].clone()
    c2d = torch.matmul(temp_Ks, poses[:, :, :3, 3].unsqueeze(-1))
    c2d = c2d / c2d[:, :, 2].unsqueeze(2)
    scale = qM[:, 0, 0]
    inv = torch.eye(3, dtype=dtype).unsqueeze(0).repeat(B, 1, 1)
    inv[:, 0, 0] = 1 / scale
    inv[:, 1, 1] = 1 / scale
    inv[:, :2, 2] = -qM[:, :2, 2] / scale.unsqueeze(1)
    if mutant == "crop_not_inverted":
        inv = qM.clone()
    inv = inv.unsqueeze(1).repeat(1, k, 1, 1)
    aff = torch.matmul(torch.matmul(inv, pM), temp_Ms)
    qc = torch.matmul(aff, c2d)
    qKs = qK[:, None].expand(B, k, 3, 3)
    iK = torch.inverse(qKs)
    scale2d = torch.norm((pM if mutant == "scale_from_pred_M" else aff)[:, :, :2, 0], dim=2)
    focal = temp_Ks[:, :, 0, 0] / qKs[:, :, 0, 0] if mutant == "focal_ratio_inverted" else qKs[:, :, 0, 0] / temp_Ks[:, :, 0, 0]
    qz = (temp_z / scale2d) * focal
    qt = torch.matmul(iK, qc).squeeze(-1)
    qt = qt / qt[:, :, 2].unsqueeze(-1)
    poses[:, :, :3, 3] = qt * qz.unsqueeze(-1)
    return poses.numpy()


def recovery_errors(got, ref64):
    """(largest rotation-entry error, largest |R^T R - I| entry, largest |dt| / |t|) of `got` (B,k,4,4) against float64."""
    got = np.asarray(got, np.float64)
    R = got[..., :3, :3]
    rot = np.abs(R - ref64[..., :3, :3]).max()
    orth = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max()
    t64 = ref64[..., :3, 3]
    trans = (np.linalg.norm(got[..., :3, 3] - t64, axis=-1) / np.linalg.norm(t64, axis=-1)).max()
    return float(rot), float(orth), float(trans)


@functools.lru_cache(maxsize=None)
def recovery_bounds(B, k):
    """(float64 poses, rotation bound, translation bound, the f32 evaluation's own errors): max(2 x the f32 evaluation's error, floor)."""
    case = recovery_case(B, k)
    ref64 = recover_restated(case)
    e32 = recovery_errors(recover_restated(case, torch.float32), ref64)
    return ref64, max(2 * e32[0], ROT_FLOOR), max(2 * e32[2], TRANS_FLOOR), e32


def recovery_check(got, B, k):
    """None, or what is wrong with (B,k,4,4) poses of recovery_case(B, k)."""
    ref64, rot_b, trans_b, _ = recovery_bounds(B, k)
    got = np.asarray(got)
    if not np.isfinite(got).all():
        return "non-finite pose entries"
    rot, orth, trans = recovery_errors(got, ref64)
    if rot > rot_b:
        return f"rotation entries off by {rot:.3g} > {rot_b:.3g}"
    if orth > rot_b:
        return f"|R^T R - I| = {orth:.3g} > {rot_b:.3g}"
    if trans > trans_b:
        return f"|dt| / |t| = {trans:.3g} > {trans_b:.3g}"
    lab, ids = recovery_case(B, k)["labels0"], recovery_case(B, k)["id_src"]
    row3 = recovery_case(B, k)["tmpl_pose"][lab[:, None], ids][..., 3, :]
    if got.dtype == np.float32 and not np.array_equal(got[..., 3, :].view(np.uint32), row3.view(np.uint32)):
        return "row 3 is not the template pose's, bit for bit"
    return None


# ================================================================================================================ ranking
RANK_MUTANTS = ("ties_higher_index", "integer_division")


def rank_restated(isc, sort=True, mutant=None):
    """gigaPose.py:588-594: score = sum(ransac_scores, dim=2) / P (int64 -> float32, true division), a stable descending sort.
    -> (scores in the returned order (B,k) f32, order (B,k) int64)."""
    isc = torch.from_numpy(np.array(isc))
    B, k, Pn = isc.shape
    s = torch.sum(isc, dim=2)
    score = (s // Pn).float() if mutant == "integer_division" else s / Pn
    assert score.dtype == torch.float32
    if not sort:
        return score.numpy(), np.broadcast_to(np.arange(k), (B, k)).copy()
    if mutant == "ties_higher_index":
        order = (k - 1 - torch.sort(score.flip(1), dim=1, descending=True, stable=True).indices)
    else:
        order = torch.sort(score, dim=1, descending=True, stable=True).indices
    return torch.gather(score, 1, order).numpy(), order.numpy()


@functools.lru_cache(maxsize=None)
def rank_scores_case(k, Pn, B=6):
    """(B,k,Pn) int64 inlier scores: random 0 / 1; an exact tie; an all-equal row; sums beyond 2^24 where different integers round to
    the same f32 and the LARGER integer sits at the higher index (a tie: the lower index goes first); negative sums; mixed signs."""
    rs = np.random.RandomState(17 * k + Pn)
    isc = (rs.uniform(size=(B, k, Pn)) < 0.3).astype(np.int64)
    isc[1] = 1
    if k > 1:
        isc[0, k - 1] = isc[0, 0]
        big = -(-(2 ** 25) // Pn)
        isc[2] = big
        isc[2, :, 0] += np.arange(k) % 3                       # sums 2^25 + {0, 1, 2} (+ slack): the same f32, integers rising with the index
        isc[3] = -isc[3] * rs.randint(1, 5, (k, Pn))
        isc[4] = rs.randint(-3, 4, (k, Pn))
        isc[4, 0, 0] += 4 * Pn
        isc[4, k - 1, 0] -= 4 * Pn
        isc[5, :, :] = 0
        isc[5, :, Pn - 1] = np.arange(k)[::-1] // 2             # the score sits in the last element alone; pairs of equal sums
    isc.setflags(write=False)
    return isc


def rank_payload_expected(src, order):
    """src (B,k,row_bytes) uint8, order (B,k): row j of the source lands at its rank."""
    return np.take_along_axis(src, order[:, :, None], 1)


# ============================================================================================================ top-k / select
TOPK_MUTANTS = ("ties_higher_index", "winners_in_index_order")
TOPK_N = (1, 63, 64, 65, 128, 162, 1000)


def topk_restated(sim, k, mutant=None):
    """torch.topk(sim_avg, k, dim=1) with the project's tie rule: lexsort on (-score, index).  -> ids (B,k) int64, scores (B,k) f32."""
    sim = np.asarray(sim, np.float32)
    idx = np.arange(sim.shape[1])
    order = np.stack([np.lexsort((-idx if mutant == "ties_higher_index" else idx, -row)) for row in sim])[:, :k]
    if mutant == "winners_in_index_order":
        order = np.sort(order, axis=1)
    return order.astype(np.int64), np.take_along_axis(sim, order, 1)


@functools.lru_cache(maxsize=None)
def topk_case(N):
    """(7, N) f32 rows: random; all equal; exact ties across the 64-lane stride (equal values at n, n + 64, n + 1); all negative;
    -0.0 against +0.0 (and nothing larger); the maximum at N - 1; a descending ramp with its tail tied."""
    rs = np.random.RandomState(N)
    x = rs.uniform(0, 1, (7, N)).astype(np.float32)
    x[1] = 0.375
    for n in (0, 5, 63):
        for m in (n, n + 64, n + 1):
            if m < N:
                x[2, m] = np.float32(2.0 + n)
    x[3] = -x[3] - 0.5
    x[4] = np.where(rs.uniform(size=N) < 0.5, np.float32(-0.0), np.float32(0.0))
    x[4, N // 2] = -1.0 if N > 2 else x[4, N // 2]
    x[5, N - 1] = 7.0
    x[6] = np.maximum(np.float32(1.0) - np.arange(N, dtype=np.float32) / 64, np.float32(-1.0))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def select_records_case(N, B=7):
    """The matcher's per-template records behind topk_case(N): idx (B,N,256) u8, score and mask (B,N,256) f32 (a third of the mask 0,
    fractional values and -0.0 among the rest: torch.nonzero keeps whatever is not zero)."""
    rs = np.random.RandomState(5000 + N)
    idx = rs.randint(0, 256, (B, N, P)).astype(np.uint8)
    sc = rs.uniform(-1, 1, (B, N, P)).astype(np.float32)
    ma = rs.choice(np.array([0.0, 1.0, 0.25, -0.0], np.float32), (B, N, P), p=[0.3, 0.5, 0.1, 0.1])
    for a in (idx, sc, ma):
        a.setflags(write=False)
    return idx, sc, ma


def format_prediction_restated(mask, input_pts):
    """LocalSimilarity.format_prediction: mask (B,k,16,16), input_pts (B,k,16,16,2) -> grid points and input points, -1 outside."""
    B, k = mask.shape[:2]
    b, n, h, w = np.nonzero(mask)
    grid_pts = np.full((B, k, G, G, 2), -1, np.int64)
    in_pts = np.full((B, k, G, G, 2), -1, np.int64)
    grid_pts[b, n, h, w] = np.stack([w, h], 1)
    in_pts[b, n, h, w] = input_pts[b, n, h, w]
    return grid_pts.reshape(B, k, P, 2), in_pts.reshape(B, k, P, 2)


def select_restated(sim, idx, sc, ma, k, mutant=None):
    """matching.py:279-316: topk, the winners' records, convert_index2location, format_prediction.
    -> ids, scores, score_pts (B,k,256), tar_pts, src_pts (B,k,256,2)."""
    ids, scores = topk_restated(sim, k, mutant)
    take = lambda a: np.take_along_axis(a, ids[:, :, None], 1)
    rec_idx, rec_mask = take(idx).astype(np.int64), take(ma)
    loc = np.stack([rec_idx % G, rec_idx // G], -1)
    tar_pts, src_pts = format_prediction_restated(rec_mask.reshape(-1, k, G, G), loc.reshape(-1, k, G, G, 2))
    return ids, scores, take(sc), tar_pts, src_pts
