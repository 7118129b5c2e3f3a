"""CPU: the host half of the detection-scoring stage (gigapose_amd/detections.py, libgigapose_coco.so, include/gigapose_coco.h).

The numpy restatement of the header (gigapose_testing/coco_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_coco.py); here it is held to readings that cannot share its mistakes: the intersections to `(a & b).sum()` on
decoded masks and to sets of pixel indices; the matching to a transcription of pycocotools' loop with fractions.Fraction IoUs; the
AP to Fraction arithmetic on rankings, one of them worked out by hand.  Eight subtly wrong versions fail these checks.  Beside
that: the product's average_precision against the restatement's, the library against its header, and every refusal, message by
message, which needs no device."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, detections
from gigapose_testing import coco_cases as cases
from gigapose_testing import coco_ref as ref
from gigapose_testing.symbols import exported_symbols

SMALL_FRAMES = ((1, 1), (1, 37), (37, 1), (48, 64))


# ---------------------------------------------------------------------------------------------- intersections
def intersections_hold(variant, frames=SMALL_FRAMES, sets=True):
    ok = True
    for H, W in frames:
        HW = H * W
        names, lists = cases.frame_lists(H, W)
        cum, offsets = cases.pack_cum(lists)
        dense = np.stack([cases.decode(c, HW) for c in lists])
        fg, area, status = ref.fg_scan(cum, offsets, HW, variant=variant)
        ok &= not status.any() and area.tolist() == dense.sum(axis=1).tolist()
        for d, c in enumerate(lists):                                  # fg[i]: the foreground pixels up to the end of run i
            ends = np.cumsum(np.asarray(c, np.int64))
            ok &= fg[offsets[d]:offsets[d + 1]].tolist() == [int(dense[d, :e].sum()) for e in ends]
        a, b = cases.every_pair(len(lists))
        inter, pstatus = ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), HW, a, b, variant)
        want = (dense[:, None, :] & dense[None, :, :]).sum(axis=2).reshape(-1)
        ok &= not pstatus.any() and inter.tolist() == want.tolist()
        if sets and HW <= 64:
            pixels = [set(np.flatnonzero(m).tolist()) for m in dense]
            ok &= inter.tolist() == [len(pixels[i] & pixels[j]) for i, j in zip(a, b)]
    return bool(ok)


def test_the_restated_intersections_equal_dense_masks_and_pixel_sets():
    assert intersections_hold(None)
    names, lists = cases.frame_lists(48, 64)
    assert sorted({len(c) for c in lists} & set(cases.RUN_COUNTS)) == list(cases.RUN_COUNTS)       # every length is there
    cum, offsets = cases.pack_cum(lists)
    fg, area, _ = ref.fg_scan(cum, offsets, 48 * 64)
    n = len(lists) // 2
    a = np.arange(n, dtype=np.int32)
    same, _ = ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), 48 * 64, a, a)
    other, _ = ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), 48 * 64, a, a + n)
    assert same.tolist() == area[:n].tolist() and not other.any()                                  # A with A, A with its complement
    i, j = names.index("a block of runs"), names.index("begins where the block's runs end")
    assert ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), 48 * 64, [i], [j])[0].tolist() == [0]


def test_the_restatement_flags_bad_masks_and_pairs_out_of_range():
    lists = [np.asarray(c, np.int32) for c in ([3, 2, 1], [6], [0, 6], [2, 2])]                    # the last one sums to 4, not 6
    cum, offsets = cases.pack_cum(lists)
    cum[offsets[2] - 1] = -1                                                                       # what a failed scan leaves
    before = np.full(len(cum), 77, np.int32)
    fg, area, status = ref.fg_scan(cum, offsets, 6, before)
    assert status.tolist() == [0, ref.BAD_MASK, 0, ref.BAD_MASK] and area.tolist() == [2, 0, 6, 0]
    assert fg.tolist() == [0, 2, 2, 77, 0, 6, 77, 77]                                              # a BAD mask's part is not written
    inter, pstatus = ref.mask_inter((cum, offsets, fg), (cum, offsets, fg), 6, [0, 0, -1, 0, 4, 2], [2, 1, 0, 3, 0, 0])
    assert pstatus.tolist() == [0, ref.PAIR_MASK, ref.PAIR_RANGE, ref.PAIR_MASK, ref.PAIR_RANGE, 0] and inter.tolist() == [2, 0, 0, 0, 0, 2]
    empty = ref.fg_scan(cum, np.asarray([0, 0, 9], np.int32), 6)
    assert empty[2].tolist() == [ref.BAD_MASK, ref.BAD_MASK]


def test_the_restated_box_intersections_equal_pixel_sets():
    rs = np.random.RandomState(5)
    box = rs.randint(-3, 12, (30, 4)).astype(np.int32)
    cells = [{(x, y) for x in range(b[0], b[2]) for y in range(b[1], b[3])} for b in box.tolist()]
    a, b = cases.every_pair(30)
    inter, area_a, area_b, status = ref.box_inter(box, box, a, b)
    assert inter.tolist() == [len(cells[i] & cells[j]) for i, j in zip(a, b)] and not status.any()
    assert area_a.tolist() == [len(cells[i]) for i in a] and area_b.tolist() == [len(cells[j]) for j in b]
    far = np.asarray([(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (0, 0, 2 ** 22, 5)], np.int32)
    inter, area_a, _, status = ref.box_inter(far, far, [0, 1, 2], [1, 1, 0])
    assert inter.tolist() == [5 << 21, 5 << 21, 0] and area_a.tolist() == [1 << 44, 5 << 21, 0] and status.tolist() == [0, 0, ref.PAIR_RANGE]


# ---------------------------------------------------------------------------------------------- matching
def coco_loop(inter, area_det, area_gt, ignore, thr):
    """pycocotools' evaluateImg loop (no crowds), IoUs as Fractions, the threshold a Fraction: -> (matches, ignore flags)."""
    D, G = len(area_det), len(area_gt)
    iou = [[Fraction(inter[d][g], area_det[d] + area_gt[g] - inter[d][g]) if area_det[d] + area_gt[g] - inter[d][g] > 0 else None for g in range(G)]
           for d in range(D)]
    gtm, dtm, dti = [False] * G, [], []
    for d in range(D):
        best, m = thr, -1
        for g in range(G):
            if gtm[g]:
                continue
            if m > -1 and not ignore[m] and ignore[g]:
                break
            if iou[d][g] is None or iou[d][g] < best:
                continue
            best, m = iou[d][g], g
        dtm.append(m), dti.append(int(bool(ignore[m])) if m > -1 else 0)
        if m > -1:
            gtm[m] = True
    return dtm, dti


def matching_holds(variant, seeds=(0, 1)):
    ok = True
    for name, inter, area_det, area_gt, ignore, want in cases.planted_groups():
        got = ref.match_group(inter, area_det, area_gt, ignore, 10, 20, variant)
        ok &= got[0] == want and got == coco_loop(inter, area_det, area_gt, ignore, Fraction(1, 2))
    rs = np.random.RandomState(11)
    for _ in range(60):
        inter, area_det, area_gt, ignore = (a.tolist() for a in cases.random_group(rs, int(rs.randint(0, 7)), int(rs.randint(0, 9)), spread=3))
        for num in (0, 10, 15, 20):
            ok &= ref.match_group(inter, area_det, area_gt, ignore, num, 20, variant) == coco_loop(inter, area_det, area_gt, ignore, Fraction(num, 20))
    return bool(ok)


def test_the_restated_matching_equals_the_loop_of_pycocotools_in_fractions():
    assert matching_holds(None)
    case = cases.assemble([g[1:5] for g in cases.planted_groups()] + cases.size_groups()[:8])
    dt_match, dt_ignore, status = ref.match(*cases.match_args(case), cases.THRESHOLDS, cases.THR_DEN)
    assert not status.any() and dt_match.shape == (10, len(case["area_det"]))
    q = 0
    for name, inter, area_det, area_gt, ignore, want in cases.planted_groups():                    # the flat form reads the same groups
        d0, d1 = case["det_off"][q:q + 2]
        assert dt_match[0, d0:d1].tolist() == want, name
        for t, num in enumerate(cases.THRESHOLDS):
            assert (dt_match[t, d0:d1].tolist(), dt_ignore[t, d0:d1].tolist()) == coco_loop(inter, area_det, area_gt, ignore, Fraction(num, 20)), (name, num)
        q += 1


def test_the_restated_matching_flags_groups_it_cannot_take():
    good = ([[5]], [5], [5], [0])
    case = cases.assemble([good, ([[5, 5]], [5], [5, 5], [1, 0]), good, good])
    case["pair_off"][3] = 99                                                                       # leaves inter
    before = np.full((1, 4), 7, np.int32), np.full((1, 4), 7, np.uint8)
    m, f, status = ref.match(*cases.match_args(case), [10], 20, dt_match=before[0], dt_ignore=before[1])
    assert status.tolist() == [0, ref.GROUP_ORDER, 0, ref.GROUP_RANGE]
    assert m.tolist() == [[0, -1, 0, 7]] and f.tolist() == [[0, 0, 0, 7]]
    big = cases.assemble([(np.zeros((1, 4097), np.int64), [3], [3] * 4097, [0] * 4097)])
    assert ref.match(*cases.match_args(big), [10], 20)[2].tolist() == [ref.GROUP_SIZE]


# ---------------------------------------------------------------------------------------------- AP
def fraction_ap(groups, T):
    """{(category, t): (AP as a Fraction, the 101 precisions as Fractions)} straight from COCO's definition."""
    out = {}
    for c in sorted({g["category"] for g in groups}):
        mine = [g for g in groups if g["category"] == c]
        npig = sum(g["npig"] for g in mine)
        if not npig:
            continue
        for t in range(T):
            rows = [(float(s), bool(m >= 0), bool(i)) for g in mine for s, m, i in zip(g["scores"], g["dt_match"][t], g["dt_ignore"][t])]
            rows = [r for r in sorted(rows, key=lambda r: -r[0]) if not r[2]]
            tp = fp = 0
            points = []                                                                            # (recall, precision)
            for _, hit, _ in rows:
                tp, fp = tp + hit, fp + (not hit)
                points.append((Fraction(tp, npig), Fraction(tp, tp + fp)))
            prec = [max((p for r, p in points if r >= Fraction(i, 100)), default=Fraction(0)) for i in range(101)]
            out[(c, t)] = (sum(prec) / 101, prec)
    return out


def ap_holds(variant, implementation=None):
    ok = True
    run = implementation or (lambda g, t, d: ref.average_precision(g, t, d, variant))
    for seed in range(4):
        groups = cases.ranking_groups(seed)
        got, want = run(groups, (10, 15, 19), 20), fraction_ap(groups, 3)
        ok &= sorted(got["cells"]) == sorted(want)
        for key in want:
            ok &= abs(got["cells"][key][0] - float(want[key][0])) <= 2.0 ** -50
            if len(got["cells"][key]) > 2:
                ok &= got["cells"][key][2] == [float(p) for p in want[key][1]]                     # each precision: one rounding
    toy = run(cases.one_cell(*cases.TOY), (10,), 20)
    ok &= toy["AP"] == math.fsum([1.0] * 51 + [2 / 3] * 50) / 101 and abs(toy["AP"] - 253 / 303) < 1e-15 and toy["AR"] == 1.0
    # 57 of 100 ground truths found by 57 detections, then one miss, then a hit: level 57 is reached at rank 56 on integers
    # (100 * 57 >= 57 * 100) at precision 1; 57 * 0.01 is 0.5700000000000001 > 57 / 100, which would read rank 58: 58 / 59
    edge = run(cases.one_cell([1] * 57 + [0, 1], 100), (10,), 20)
    ok &= edge["AP"] == math.fsum([1.0] * 58 + [58 / 59] + [0.0] * 42) / 101
    return bool(ok)


def test_the_restated_ap_equals_fraction_arithmetic_and_the_toy_worked_by_hand():
    assert ap_holds(None)
    out = ref.average_precision(cases.ranking_groups(0), (10, 15, 19), 20)
    assert 9 not in out["per_category"] and 5 in out["per_category"]                               # npig == 0 is left out; no detections: AP 0
    assert out["per_category"][5]["AP"] == 0.0 and out["AP75"] == ref._mean(v[0] for k, v in out["cells"].items() if k[1] == 1)
    assert out["AP50"] == ref._mean(v[0] for k, v in out["cells"].items() if k[1] == 0)
    assert ref.average_precision([], (10,), 20)["AP"] == -1.0
    ignored = ref.average_precision(cases.one_cell([1, 1, 0, 1], 2, ignored=[0, 1, 1, 0]), (10,), 20)       # ignored detections are dropped
    assert ignored["AP"] == 1.0
    ties = ref.average_precision(cases.one_cell([0, 1], 1, scores=[0.5, 0.5]), (10,), 20)          # a stable sort: the miss stays first
    assert ties["AP"] == 0.5


def test_the_products_average_precision_equals_the_restatement_and_the_fractions():
    assert ap_holds(None, detections.average_precision)
    for seed in range(4):
        groups = cases.ranking_groups(seed)
        got, want = detections.average_precision(groups, (10, 15, 19), 20), ref.average_precision(groups, (10, 15, 19), 20)
        for name in ("AP", "AP50", "AP75", "AR", "per_category"):
            assert got[name] == want[name], name
        assert {k: v[:2] for k, v in want["cells"].items()} == got["cells"]
    assert detections.average_precision([], (10,), 20)["AP"] == -1.0
    with pytest.raises(ValueError, match="is NaN"):
        detections.average_precision(cases.one_cell([1], 1, scores=[float("nan")]), (10,), 20)
    with pytest.raises(ValueError, match="1 scores for 2 matches"):
        detections.average_precision([dict(category=1, scores=[0.5], dt_match=np.zeros((1, 2), np.int32), dt_ignore=np.zeros((1, 2), np.uint8), npig=1)], (10,), 20)


# ---------------------------------------------------------------------------------------------- the wrong versions
def checks_pass(variant):
    return intersections_hold(variant, frames=((1, 37), (48, 64)), sets=False) and matching_holds(variant) and ap_holds(variant)


def test_the_checks_hold_for_the_restatement():
    assert checks_pass(None)
    assert all(checks_pass(v) for v in ref.HARMLESS)                   # F is continuous at a run's end: see coco_ref.HARMLESS


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_checks_reject_wrong_versions(variant):
    assert len(ref.VARIANTS) >= 7 and not checks_pass(variant)


def test_evaluate_scores_perfect_duplicated_and_ignored_detections():
    H, W = 4, 6
    a, b = [2, 6, 16], [12, 8, 4]                                      # two masks that do not meet
    gt = lambda counts, c, ignore=False: dict(category=c, ignore=ignore, cum=np.cumsum(counts))     # noqa: E731
    det = lambda counts, c, s: dict(category=c, score=s, cum=np.cumsum(counts))                    # noqa: E731
    perfect = ref.evaluate([([gt(a, 1), gt(b, 2)], [det(a, 1, 0.9), det(b, 2, 0.8)])], HW=H * W)
    assert perfect["AP"] == 1.0 and perfect["AR"] == 1.0
    dup = ref.evaluate([([gt(a, 1)], [det(a, 1, 0.9), det(a, 1, 0.8)])], HW=H * W)                 # the duplicate is a late false positive
    assert dup["AP"] == 1.0
    wrong = ref.evaluate([([gt(a, 1)], [det(a, 2, 0.9)])], HW=H * W)
    assert wrong["AP"] == 0.0 and sorted(wrong["per_category"]) == [1]
    seen = ref.evaluate([([gt(a, 1), gt(b, 1, True)], [det(b, 1, 0.9), det(a, 1, 0.8)])], HW=H * W)       # the ignored one is neither missed nor false
    assert seen["AP"] == 1.0 and seen["AR"] == 1.0
    boxes = ref.evaluate([([dict(category=1, ignore=False, box=[0, 0, 4, 4])], [dict(category=1, score=1.0, box=[0, 0, 4, 2])])])
    assert boxes["AP50"] == 1.0 and boxes["AP"] == 0.1                 # IoU 1/2: met at 10/20 only


# ---------------------------------------------------------------------------------------------- the library and its header
def test_coco_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_coco.so", "gpc")        # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_coco.h" and side.path == detections.COCO_LIB_PATH
    assert sorted(protos) == ["gpc_abi_version", "gpc_box_inter", "gpc_fg_scan", "gpc_last_error", "gpc_mask_inter", "gpc_match", "gpc_sup_bits"]
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpc_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_", "gpf_", "gpv_", "gpm_", "gpl_", "gpg_", "gpa_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the coco library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    P, I = ctypes.c_void_p, ctypes.c_int
    assert list(lib.gpc_fg_scan.argtypes) == [P, P, I, I, I, P, P, P, P]
    assert list(lib.gpc_mask_inter.argtypes) == [P, P, P, I, I, P, P, P, I, I, I, P, P, I, P, P, P]
    assert list(lib.gpc_box_inter.argtypes) == [P, I, P, I, P, P, I, P, P, P, P, P]
    assert list(lib.gpc_match.argtypes) == [P, P, P, I, P, I, P, I, P, P, I, P, I, I, P, P, P, P]
    assert list(lib.gpc_sup_bits.argtypes) == [P, P, I, I, I, P, P]
    assert lib.gpc_abi_version() >= 1
    header = open(_lib.INCLUDE_DIR + "/gigapose_coco.h").read()
    for name, value, mine, restated in (("GPC_MAX_ITEMS", 65535, detections.MAX_ITEMS_PER_CALL, None), ("GPC_MAX_THRESHOLDS", 16, detections.MAX_THRESHOLDS, None),
                                        ("GPC_MAX_DEN", 65536, detections.MAX_DEN, None), ("GPC_MAX_GROUP_GT", 4096, detections.MAX_GROUP_GT, ref.MAX_GROUP_GT),
                                        ("GPC_MAX_NMS", 2048, detections.MAX_NMS, None), ("GPC_MAX_COORD", 1 << 21, None, ref.MAX_COORD),
                                        ("GPC_BAD_MASK", 1, detections.BAD_MASK, ref.BAD_MASK), ("GPC_PAIR_RANGE", 1, detections.PAIR_RANGE, ref.PAIR_RANGE),
                                        ("GPC_PAIR_MASK", 2, detections.PAIR_MASK, ref.PAIR_MASK), ("GPC_GROUP_RANGE", 1, detections.GROUP_RANGE, ref.GROUP_RANGE),
                                        ("GPC_GROUP_ORDER", 2, detections.GROUP_ORDER, ref.GROUP_ORDER), ("GPC_GROUP_SIZE", 4, detections.GROUP_SIZE, ref.GROUP_SIZE)):
        assert f"#define {name} {value}" in header and mine in (None, value) and restated in (None, value), name


def test_coco_argument_validation_of_the_library_needs_no_gpu():
    lib = detections.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(8), ctypes.c_void_p(12)   # `one`: a non-null pointer that is never followed
    err = lib.gpc_last_error

    # Nothing is launched on this machine: the calls that pass are the empty ones
    def scan(total=10, D=3, HW=100, **p):
        g = {n: p.get(n, one) for n in ("cum", "offsets", "fg", "area", "status")}
        return lib.gpc_fg_scan(g["cum"], g["offsets"], total, D, HW, g["fg"], g["area"], g["status"], null)

    for kw in (dict(D=-1), dict(D=65536), dict(HW=0), dict(HW=-5), dict(total=-1)):
        assert scan(**kw) == -1 and b"gpc_fg_scan" in err() and b"bad sizes" in err(), kw
    for name in ("cum", "offsets", "fg", "area", "status"):
        assert scan(**{name: null}) == -1 and b"null" in err(), name
    assert scan(area=odd) == -1 and b"aligned" in err()
    assert scan(D=0, cum=null, area=null) == 0 and scan(D=0, HW=2 ** 31 - 1, total=2 ** 31 - 1) == 0 and scan(D=0, HW=0) == -1

    def inter(totalA=10, DA=3, totalB=10, DB=3, HW=100, P=5, **p):
        g = {n: p.get(n, one) for n in ("cumA", "offA", "fgA", "cumB", "offB", "fgB", "pair_a", "pair_b", "inter", "status")}
        return lib.gpc_mask_inter(g["cumA"], g["offA"], g["fgA"], totalA, DA, g["cumB"], g["offB"], g["fgB"], totalB, DB, HW, g["pair_a"],
                                  g["pair_b"], P, g["inter"], g["status"], null)

    for kw, msg in ((dict(P=-1), b"pairs"), (dict(P=65536), b"pairs"), (dict(DA=-1), b"bad sizes"), (dict(DB=-1), b"bad sizes"),
                    (dict(totalA=-1), b"bad sizes"), (dict(totalB=-1), b"bad sizes"), (dict(HW=0), b"bad sizes")):
        assert inter(**kw) == -1 and b"gpc_mask_inter" in err() and msg in err(), kw
    for name in ("cumA", "offA", "fgA", "cumB", "offB", "fgB", "pair_a", "pair_b", "inter", "status"):
        assert inter(**{name: null}) == -1 and b"null" in err(), name
    assert inter(inter=odd) == -1 and b"aligned" in err()
    assert inter(P=0, cumA=null, inter=null) == 0 and inter(P=0, HW=0) == -1

    def boxes(DA=3, DB=3, P=5, **p):
        g = {n: p.get(n, one) for n in ("boxA", "boxB", "pair_a", "pair_b", "inter", "area_a", "area_b", "status")}
        return lib.gpc_box_inter(g["boxA"], DA, g["boxB"], DB, g["pair_a"], g["pair_b"], P, g["inter"], g["area_a"], g["area_b"], g["status"], null)

    for kw, msg in ((dict(P=-1), b"pairs"), (dict(P=65536), b"pairs"), (dict(DA=-1), b"bad sizes"), (dict(DB=-1), b"bad sizes")):
        assert boxes(**kw) == -1 and b"gpc_box_inter" in err() and msg in err(), kw
    for name in ("boxA", "boxB", "pair_a", "pair_b", "inter", "area_a", "area_b", "status"):
        assert boxes(**{name: null}) == -1 and b"null" in err(), name
    for name in ("inter", "area_a", "area_b"):
        assert boxes(**{name: odd}) == -1 and b"aligned" in err(), name
    assert boxes(P=0, boxA=null, inter=null) == 0

    def match(Q=2, total_pair=4, total_det=4, total_gt=4, T=10, den=20, **p):
        g = {n: p.get(n, one) for n in ("det_off", "gt_off", "pair_off", "inter", "area_det", "area_gt", "gt_ignore", "thr_num", "dt_match", "dt_ignore", "status")}
        return lib.gpc_match(g["det_off"], g["gt_off"], g["pair_off"], Q, g["inter"], total_pair, g["area_det"], total_det, g["area_gt"], g["gt_ignore"],
                             total_gt, g["thr_num"], T, den, g["dt_match"], g["dt_ignore"], g["status"], null)

    for kw, msg in ((dict(Q=-1), b"groups"), (dict(Q=65536), b"groups"), (dict(T=0), b"thresholds"), (dict(T=17), b"thresholds"), (dict(den=0), b"thr_den"),
                    (dict(den=65537), b"thr_den"), (dict(total_pair=-1), b"bad sizes"), (dict(total_det=-1), b"bad sizes"), (dict(total_gt=-1), b"bad sizes")):
        assert match(**kw) == -1 and b"gpc_match" in err() and msg in err(), kw
    for name in ("det_off", "gt_off", "pair_off", "inter", "area_det", "area_gt", "gt_ignore", "thr_num", "dt_match", "dt_ignore", "status"):
        assert match(**{name: null}) == -1 and b"null" in err(), name
    for name in ("inter", "area_det", "area_gt"):
        assert match(**{name: odd}) == -1 and b"aligned" in err(), name
    assert match(Q=0, det_off=null) == 0 and match(Q=0, T=16, den=65536) == 0 and match(Q=0, T=0) == -1

    def bits(P=5, num=1, den=4, inter=one, area=one, sup=one):
        return lib.gpc_sup_bits(inter, area, P, num, den, sup, null)

    for kw, msg in ((dict(P=-1), b"masks"), (dict(P=2049), b"masks"), (dict(num=-1), b"threshold"), (dict(num=5), b"threshold"), (dict(den=0, num=0), b"threshold"),
                    (dict(den=65537), b"threshold")):
        assert bits(**kw) == -1 and b"gpc_sup_bits" in err() and msg in err(), kw
    for name in ("inter", "area", "sup"):
        assert bits(**{name: null}) == -1 and b"null" in err(), name
        assert bits(**{name: odd}) == -1 and b"aligned" in err(), name
    assert bits(P=0, inter=null, sup=null) == 0 and bits(P=0, num=65536, den=65536) == 0


def test_coco_argument_validation_of_the_python_layer_needs_no_gpu():
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    cum, offsets = torch.tensor([2, 6], dtype=i32), torch.tensor([0, 2], dtype=i32)
    for a, match in ((((cum, offsets, cum), 6), r"must be \(cum, offsets\)"), (((cum.long(), offsets), 6), "cum"), (((cum, offsets.float()), 6), "offsets"),
                     (((cum, offsets), 0), "HW = 0"), (((cum, offsets), 2 ** 31), "HW ="), (((cum, offsets[:0]), 6), "D \\+ 1 entries")):
        with pytest.raises(ValueError, match=match):
            detections.foreground(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        detections.foreground((cum, offsets), 6)
    fg = detections.Foreground(cum, offsets, cum, torch.zeros(1, dtype=i64), torch.zeros(1, dtype=i32), 6)
    other = detections.Foreground(cum, offsets, cum, torch.zeros(1, dtype=i64), torch.zeros(1, dtype=i32), 8)
    pair = torch.zeros(3, dtype=i32)
    for a, match in (((fg, (cum, offsets), pair, pair), "must be Foregrounds"), ((fg, other, pair, pair), "frames of 6 and 8 pixels"),
                     ((fg, fg, pair.long(), pair), "pair_a"), ((fg, fg, pair, pair[:2]), "pair_b")):
        with pytest.raises(ValueError, match=match):
            detections.mask_intersections(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        detections.mask_intersections(fg, fg, pair, pair)
    box = torch.zeros(4, 4, dtype=i32)
    for a, match in (((box.long(), box, pair, pair), "box_a"), ((box, box[:, :3], pair, pair), "box_b"), ((box, box, pair, pair[:1]), "pair_b")):
        with pytest.raises(ValueError, match=match):
            detections.box_intersections(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        detections.box_intersections(box, box, pair, pair)
    g = dict(det_off=torch.tensor([0, 1], dtype=i32), gt_off=torch.tensor([0, 1], dtype=i32), pair_off=torch.zeros(1, dtype=i32), inter=torch.ones(1, dtype=i64),
             area_det=torch.ones(1, dtype=i64), area_gt=torch.ones(1, dtype=i64), gt_ignore=torch.zeros(1, dtype=u8), thresholds=(10,), thr_den=20)
    for kw, match in ((dict(thresholds=()), "0 thresholds"), (dict(thresholds=range(17)), "17 thresholds"), (dict(thresholds=(21,)), "bad IoU thresholds"),
                      (dict(thr_den=0), "bad IoU thresholds"), (dict(thresholds=(-1,)), "bad IoU thresholds"), (dict(gt_off=g["gt_off"][:1]), "Q \\+ 1 entries"),
                      (dict(pair_off=torch.zeros(2, dtype=i32)), "pair_off"), (dict(inter=g["inter"].int()), "inter"), (dict(area_det=g["area_det"].int()), "area_det"),
                      (dict(gt_ignore=torch.zeros(2, dtype=u8)), "gt_ignore"), (dict(det_off=g["det_off"].long()), "det_off")):
        with pytest.raises(ValueError, match=match):
            detections.match(**dict(g, **kw))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        detections.match(**g)
    inter, area = torch.zeros(3, 3, dtype=i64), torch.zeros(3, dtype=i64)
    for a, match in (((inter[:2], area, 1, 4), "inter"), ((inter, area.int(), 1, 4), "area"), ((inter, area, 5, 4), "threshold"),
                     ((torch.zeros(2049, 2049, dtype=i64), torch.zeros(2049, dtype=i64), 1, 4), "limit is 2048")):
        with pytest.raises(ValueError, match=match):
            detections.sup_bits(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        detections.sup_bits(inter, area, 1, 4)
    order = torch.zeros(1, dtype=i64)
    for a, match in ((((cum, offsets), order, 1, 4), "must be a Foreground"), ((fg, order.int(), 1, 4), "order"), ((fg, order, 1, 0), "threshold"),
                     ((fg, torch.zeros(2049, dtype=i64), 1, 4), "limit is 2048"), ((fg, order, 1, 4, torch.zeros(2, dtype=i32)), "label")):
        with pytest.raises(ValueError, match=match):
            detections.mask_nms(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        detections.mask_nms(fg, order, 1, 4)
    from gigapose_amd import proposals
    with pytest.raises(ValueError, match=r"expected sup \(P, \(P \+ 63\) // 64\)"):
        proposals.nms_keep(torch.zeros(3, 2, dtype=i64))
    with pytest.raises(ValueError, match="nms_on must be 'box' or 'mask'"):
        proposals.ProposalLabeller(None, None, nms_on="iou")


def test_the_scorer_refuses_what_it_cannot_score_without_a_gpu():
    seg = dict(size=[2, 3], counts=[1, 2, 3])
    row = dict(obj_id=4, visib_fract=0.5, bbox_visib=[0, 0, 2, 1], bbox_obj=[0, 0, 2, 1], mask_visib=seg, mask=seg)
    gts = {(1, 1): [row]}
    for kw, match in ((dict(iou_type="keypoints"), "iou_type"), (dict(gt_mask="mask_full"), "gt_mask"), (dict(min_visib=1.5), "min_visib"), (dict(max_dets=0), "max_dets"),
                      (dict(thresholds=()), "0 thresholds"), (dict(thr_den=0), "bad IoU thresholds")):
        with pytest.raises(ValueError, match=match):
            detections.DetectionScorer(gts, **kw)
    with pytest.raises(ValueError, match="has no 'visib_fract'"):
        detections.DetectionScorer({(1, 1): [{k: v for k, v in row.items() if k != "visib_fract"}]})
    with pytest.raises(ValueError, match="has no 'obj_id'"):
        detections.DetectionScorer({(1, 1): [{k: v for k, v in row.items() if k != "obj_id"}]})
    with pytest.raises(ValueError, match="lists 1 ground truths and `objects` 2"):
        detections.DetectionScorer({(1, 1): [{k: v for k, v in row.items() if k != "obj_id"}]}, objects={(1, 1): [dict(obj_id=1), dict(obj_id=2)]})
    named = detections.DetectionScorer({(1, 1): [{k: v for k, v in row.items() if k != "obj_id"}]}, objects={(1, 1): [dict(obj_id=8)]}, min_visib=0.6)
    assert named.rows[0][1:3] == (8, True) and detections.DetectionScorer(gts, min_visib=None).rows[0][2] is False
    with pytest.raises(ValueError, match="has no 'mask'"):
        detections.DetectionScorer({(1, 1): [{k: v for k, v in row.items() if k != "mask"}]}, gt_mask="mask")
    with pytest.raises(ValueError, match="float boxes are out of scope"):
        detections.DetectionScorer({(1, 1): [dict(row, bbox_visib=[0.5, 0, 2, 1])]}, iou_type="bbox")
    det = dict(category_id=4, score=0.9, bbox=[0, 0, 2, 1], segmentation=seg)
    scorer = detections.DetectionScorer(gts, device="cpu")
    with pytest.raises(ValueError, match="NaN score"):
        scorer.score({(1, 1): [dict(det, score=float("nan"))]})
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        scorer.score({(1, 1): [det]})
    boxes = detections.DetectionScorer(gts, iou_type="bbox")
    with pytest.raises(ValueError, match="float boxes are out of scope"):
        boxes.score({(1, 1): [dict(det, bbox=[0, 0, 2.5, 1])]})
    with pytest.raises(ValueError, match="area must stay below 2\\^31"):
        boxes.score({(1, 1): [dict(det, bbox=[0, 0, 2 ** 16, 2 ** 15])]})
    segm = detections.DetectionScorer(gts)
    with pytest.raises(ValueError, match="compressed string counts"):
        segm.score({(1, 1): [dict(det, segmentation=dict(size=[2, 3], counts="06"))]})
    with pytest.raises(ValueError, match="does not match the frame size"):
        segm.score({(1, 1): [dict(det, segmentation=dict(size=[3, 2], counts=[6]))]})
    with pytest.raises(ValueError, match="needs every detection's 'segmentation'"):
        segm.score({(1, 1): [dict(det, segmentation=None)]})
