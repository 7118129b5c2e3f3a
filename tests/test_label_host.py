"""CPU: the host half of the proposal-labelling stage (gigapose_amd/proposals.py, libgigapose_label.so, include/gigapose_label.h).

The numpy restatement of the header (gigapose_testing/label_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_label.py); here it is held to readings that cannot share its mistakes: the descriptor to exact rational arithmetic
(fractions.Fraction, roots in 60-digit decimals) and to a plain float64 LayerNorm + normalise; the scores to loops in Python
integers and to float64 mean(topk(cosine)); the NMS to sets of pixels; the boxes to numpy.nonzero on decoded masks.  Seven subtly
wrong labellers fail these checks.  Beside that: the library against its header, and every refusal of the limits, message by
message, which needs no device."""
import ctypes
import decimal
from fractions import Fraction

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, proposals
from gigapose_testing import label_cases as cases
from gigapose_testing import label_ref as ref
from gigapose_testing.symbols import exported_symbols


# ---------------------------------------------------------------------------------------------- descriptors
def exact_descriptor(x, gamma, beta, eps):
    """One row in rational arithmetic; the two roots to 60 digits -> the exactly rounded q (ties cannot occur at that precision)."""
    decimal.getcontext().prec = 60
    xs, g, b = ([Fraction(float(v)) for v in a] for a in (x, gamma, beta))
    C = len(xs)
    mean = sum(xs) / C
    var = sum((v - mean) ** 2 for v in xs) / C

    def root(fr):
        return (decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)).sqrt()

    r = 1 / root(var + Fraction(float(eps)))
    y = [decimal.Decimal((v - mean).numerator) / decimal.Decimal((v - mean).denominator) * r * decimal.Decimal(float(gv)) + decimal.Decimal(float(bv))
         for v, gv, bv in zip(xs, g, b)]
    norm = sum(v * v for v in y).sqrt()
    return [int((v / norm * (1 << 20)).to_integral_value(rounding=decimal.ROUND_HALF_EVEN)) for v in y]


def float64_descriptor(x, gamma, beta, eps):
    x = np.asarray(x, np.float64)
    y = (x - x.mean(axis=1, keepdims=True)) / np.sqrt(x.var(axis=1, keepdims=True) + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return y / np.linalg.norm(y, axis=1, keepdims=True)


@pytest.mark.parametrize("C", (64, 384, 2048))
def test_descriptor_restatement_is_within_one_unit_of_the_exact_value(C):
    gamma, beta = cases.norm_parameters(C, C)
    x, kinds = cases.token_rows(C + 1, 10, C)
    q, status = ref.descriptors(x, gamma, beta, cases.EPS)
    assert q.dtype == np.int32 and status.dtype == np.int32
    with np.errstate(all="ignore"):
        plain = float64_descriptor(x, gamma, beta, cases.EPS)
    for b, kind in enumerate(kinds):
        if kind in ("nan", "inf"):
            assert status[b] == ref.NON_FINITE and not q[b].any(), kind
            continue
        assert status[b] == 0 and np.abs(q[b] - plain[b] * 2.0 ** 20).max() <= 1.0, kind
        assert abs(int((q[b].astype(np.int64) ** 2).sum()) - (1 << 40)) <= C << 20                # a unit vector, to the quantisation
        if C == 64 or b < 3:
            assert np.abs(q[b] - np.asarray(exact_descriptor(x[b], gamma, beta, cases.EPS))).max() <= 1, kind
        if kind == "constant":                                                                   # variance 0: the normalised beta
            want = beta.astype(np.float64) / np.linalg.norm(beta.astype(np.float64))
            assert np.abs(q[b] - want * 2.0 ** 20).max() <= 1.0
    assert {"random", "massive", "constant"} <= set(kinds)


def test_descriptor_restatement_is_exact_where_the_arithmetic_is():
    """x = +-1 in equal numbers, gamma = 1, beta = 0, eps = 0: mean 0, variance 1, norm sqrt(C) = 8, 16, 32 -- every step is exact."""
    for C in (64, 256, 1024):
        x = np.where(np.random.RandomState(C).permutation(C) % 2 == 0, 1.0, -1.0).astype(np.float32)[None]
        q, status = ref.descriptors(x, np.ones(C, np.float32), np.zeros(C, np.float32), 0.0)
        assert status[0] == 0 and (q[0] == x[0] * ((1 << 20) >> (int(np.log2(C)) // 2))).all()
    gamma, beta = cases.norm_parameters(2, 64, zero_beta=True)
    x, kinds = cases.token_rows(3, 5, 64)
    q, status = ref.descriptors(x, gamma, beta, cases.EPS)
    assert status[kinds.index("constant")] == ref.ZERO_NORM and not q[kinds.index("constant")].any()      # beta = 0: nothing to normalise
    assert status[kinds.index("random")] == 0


def test_descriptor_sum_follows_the_header_order():
    """The order matters in the last bit: the restated SUM equals the thread-by-thread loop, and differs from numpy's own sum somewhere."""
    rs = np.random.RandomState(5)
    v = (rs.standard_normal((40, 768)) * 10.0 ** rs.uniform(-3, 3, (40, 768)))
    got = ref.block_sum(v)
    for b in range(40):
        part = [0.0] * 256
        for t in range(256):
            for c in range(t, 768, 256):
                part[t] = part[t] + float(v[b, c])
        off = 128
        while off >= 1:
            for t in range(off):
                part[t] = part[t] + part[t + off]
            off //= 2
        assert got[b] == part[0]
    assert (got != v.sum(axis=1)).any() or (got != np.cumsum(v, axis=1)[:, -1]).any()


# ---------------------------------------------------------------------------------------------- scores
def scores_in_python(q, bank, k):
    P, (O, T, C) = len(q), bank.shape
    ql, bl = q.tolist(), bank.tolist()
    out = dict(obj=[], label=[], score=[], best_template=[])
    for p in range(P):
        dots = [[sum(a * b for a, b in zip(ql[p], bl[o][t])) for t in range(T)] for o in range(O)]
        obj = [sum(sorted(row, reverse=True)[:min(k, T)]) for row in dots]
        label = min(o for o in range(O) if obj[o] == max(obj))
        out["obj"].append(obj), out["label"].append(label), out["score"].append(obj[label])
        out["best_template"].append(min(t for t in range(T) if dots[label][t] == max(dots[label])))
    return out


SMALL_SHAPES = [(5, 1, 1, 64, 1), (4, 2, 4, 64, 5), (6, 3, 6, 64, 5), (3, 4, 7, 128, 7), (7, 5, 5, 64, 1), (2, 2, 9, 64, 64)]


@pytest.mark.parametrize("plant", cases.SCORE_PLANTS)
def test_scores_restatement_equals_a_loop_in_python_integers(plant):
    for n, (P, O, T, C, k) in enumerate(SMALL_SHAPES):
        q, bank = cases.score_case(40 + n, P, O, T, C, plant)
        assert np.abs(q).max(initial=0) <= ref.Q_ONE and np.abs(bank).max() <= ref.Q_ONE
        got, want = ref.scores(q, bank, k), scores_in_python(q, bank, k)
        for name in want:
            assert got[name].tolist() == want[name], (plant, name, (P, O, T, C, k))
        assert got["kk"] == min(k, T)
    q, bank = cases.score_case(1, 3, 2, 3, 2048, "extreme")                                       # the largest sums stay exact
    assert ref.scores(q, bank, 1)["dot"][0, 1, 2] == 2048 << 40 == scores_in_python(q, bank, 1)["score"][0]


def test_float_score_is_within_the_quantisation_bound_of_the_float64_cosine():
    """With u, v unit vectors and q = rint(2^20 u), b = rint(2^20 v): q = 2^20 u + e, b = 2^20 v + f, |e_c|, |f_c| <= 1/2, so
    q . b / 2^40 - u . v = (u . f + v . e) / 2^20 + e . f / 2^40, and |u . f| <= |u|_1 / 2 <= sqrt(C) / 2 (likewise v . e), |e . f| <= C / 4:
    the error of one dot is at most sqrt(C) 2^-20 + C 2^-42 < C 2^-20.  A mean of top-k dots moves by no more than its largest term's
    error (top-k sums are 1-Lipschitz per element in the maximum norm), so the same bound holds for the score."""
    rs = np.random.RandomState(8)
    for P, O, T, C, k in ((9, 4, 6, 64, 5), (5, 3, 4, 384, 5), (4, 2, 9, 1024, 1)):
        u, v = cases.unit_vectors(rs, P, C), cases.unit_vectors(rs, O * T, C).reshape(O, T, C)
        u = u + v[rs.randint(O, size=P), rs.randint(T, size=P)]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        got = ref.scores(cases.quantise(u), cases.quantise(v), k)
        cos = np.einsum("pc,otc->pot", u, v)
        want = -np.sort(-cos, axis=2)[:, :, :min(k, T)].mean(axis=2)
        assert np.abs(ref.float_score(got["obj"], got["kk"]) - want).max() <= C * 2.0 ** -20
        assert (got["label"] == want.argmax(axis=1)).all() and np.abs(ref.float_score(got["score"], got["kk"]) - want.max(axis=1)).max() <= C * 2.0 ** -20


# ---------------------------------------------------------------------------------------------- boxes
def test_run_boxes_restatement_equals_nonzero_on_the_decoded_masks():
    for H, W in ((1, 9), (7, 1), (5, 8), (23, 37)):
        names, masks = cases.planted_masks(H, W)
        rs = np.random.RandomState(H)
        masks = np.concatenate([masks, rs.uniform(size=(6, H, W)) < 0.3])
        lists = cases.mask_lists(masks) + [np.asarray([0, H * W], np.int32), np.asarray([3, 0, H * W - 3], np.int32)]      # zero-length runs
        for m, c in zip(masks, lists):
            assert (cases.decode(c, H, W) == m).all()
        dense = np.stack([cases.decode(c, H, W) for c in lists])
        counts, offsets = cases.pack(lists)
        cum = np.concatenate([np.cumsum(c) for c in lists]).astype(np.int32)
        box, area, status = ref.run_boxes(cum, offsets, len(cum), H, W)
        want_box, want_area = cases.dense_boxes(dense)
        assert (box == want_box).all() and (area == want_area).all(), (H, W)
        assert status.tolist() == [0 if m.any() else ref.EMPTY_MASK for m in dense]
    bad = ref.run_boxes(np.asarray([3, 7, -1], np.int32), np.asarray([0, 3, 3, 5], np.int32), 3, 2, 5)
    assert bad[2].tolist() == [ref.BAD_MASK] * 3 and not bad[0].any() and not bad[1].any()


# ---------------------------------------------------------------------------------------------- NMS
def nms_in_sets(box, label, num, den, per_label):
    """Boxes as sets of pixels, IoU as a Fraction, greedy in order."""
    cells = [{(x, y) for x in range(b[0], b[2]) for y in range(b[1], b[3])} for b in box]
    kept = []
    for j in range(len(box)):
        def hit(i):
            union = len(cells[i] | cells[j])
            return union > 0 and Fraction(len(cells[i] & cells[j]), union) > Fraction(num, den) and (not per_label or label[i] == label[j])
        if not any(hit(i) for i in kept):
            kept.append(j)
    return [int(j in kept) for j in range(len(box))]


def small_nms_case(seed, P):
    box, label = cases.nms_case(seed, P)
    return np.where(box >= 1000, box % 1000 + 3, box % 47).astype(np.int32), label          # folded into a few dozen pixels: the sets stay small


def test_nms_restatement_equals_the_set_reading():
    for P in (0, 1, 9, 40, 70):
        box, label = small_nms_case(P, P)
        box[:, 2:] = np.maximum(box[:, 2:], box[:, :2] - 2)                  # some stay inverted: empty sets
        for num, den in ((1, 4), (0, 1), (1, 1), (1, 2)):
            for per_label in (False, True):
                assert ref.nms(box, label, num, den, per_label).tolist() == nms_in_sets(box.tolist(), label.tolist(), num, den, per_label), (P, num, den)
    A = (0, 0, 5, 1)
    for name, expect in (("at", 1), ("above", 0), ("below", 1)):            # exactly at the threshold: kept
        assert ref.nms([A, cases.THRESHOLD_PAIRS[name]], None, 1, 4, False).tolist() == [1, expect]
    assert ref.nms(cases.chain(3), None, 1, 4, False).tolist() == [1, 0, 1]  # A > B > C: C stays because B went
    assert ref.nms(cases.chain(131), None, 1, 4, False).tolist() == [1 - (i & 1) for i in range(131)]
    assert ref.nms_matrix(cases.chain(66), None, 1, 4, False)[63].tolist() == [0, 1] and ref.nms_matrix(cases.chain(66), None, 1, 4, False)[62, 0] == 1 << 63


# ---------------------------------------------------------------------------------------------- the wrong versions
def checks_pass(variant):
    """The checks above in small: True when `variant` passes all of them."""
    ok = True
    q, bank = cases.score_case(3, 6, 4, 4, 64, "ties")
    got, want = ref.scores(q, bank, 5, variant), scores_in_python(q, bank, 5)
    ok &= all(got[n].tolist() == want[n] for n in want)
    q1 = cases.quantise(cases.unit_vectors(np.random.RandomState(1), 1, 64))
    self_match = ref.scores(q1, np.repeat(q1[None], 4, axis=1), 5, variant)                       # T = 4 < k: the mean of 4 equal dots is 1
    ok &= abs(float(ref.float_score(self_match["score"], self_match["kk"])[0]) - 1.0) <= 64 * 2.0 ** -20
    q, bank = cases.score_case(4, 5, 3, 6, 64, "negative")
    bank[:, 0] = -bank[:, 1]                                                                     # one large positive dot among negative ones
    got, want = ref.scores(q, bank, 2, variant), scores_in_python(q, bank, 2)
    ok &= got["obj"].tolist() == want["obj"]
    box = [(0, 0, 5, 1), cases.THRESHOLD_PAIRS["at"]]
    ok &= ref.nms(box, None, 1, 4, False, variant).tolist() == [1, 1]
    ok &= ref.nms(cases.chain(3), None, 1, 4, False, variant).tolist() == [1, 0, 1]
    H, W = 5, 8
    _, masks = cases.planted_masks(H, W)
    lists = cases.mask_lists(masks)
    counts, offsets = cases.pack(lists)
    cum = np.concatenate([np.cumsum(c) for c in lists]).astype(np.int32)
    ok &= bool((ref.run_boxes(cum, offsets, len(cum), H, W, variant)[0] == cases.dense_boxes(masks)[0]).all())
    return bool(ok)


def test_the_checks_hold_for_the_restatement():
    assert checks_pass(None)


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_checks_reject_wrong_versions(variant):
    assert len(ref.VARIANTS) >= 6 and not checks_pass(variant)


def test_label_proposals_orders_drops_and_cuts():
    sc = dict(score=np.asarray([5, 9, 9, 1, 7, 9], np.int64) << 38, label=np.asarray([0, 1, 1, 0, 0, 1], np.int32))
    box = [(0, 0, 4, 4), (10, 0, 14, 4), (10, 0, 14, 4), (20, 0, 24, 4), (0, 0, 4, 4), (30, 0, 34, 4)]
    kept, report = ref.label_proposals([0, 0, 0, 0, 0, 1], sc, [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1], box, 1, 0.5, (1, 4), False, 2, 2)
    # image 0: 1 and 2 tie (the lower index first, 2 is its duplicate), 0 follows, 3 is below 0.5 (1/4), 4 is flagged; image 1: an empty mask
    assert kept == [[1, 0], []] and report == dict(proposals=6, empty_mask=1, flagged_descriptor=1, low_score=1, suppressed=1, over_max_dets=0, kept=2)
    kept, report = ref.label_proposals([0] * 6, sc, [0] * 6, [0] * 6, box, 1, 0.0, (1, 1), False, 3, 1)
    assert kept == [[1, 2, 5]] and report["over_max_dets"] == 3


# ---------------------------------------------------------------------------------------------- the library and its header
def test_label_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_label.so", "gpa")       # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_label.h" and side.path == proposals.LABEL_LIB_PATH
    assert sorted(protos) == ["gpa_abi_version", "gpa_descriptors", "gpa_last_error", "gpa_nms_keep", "gpa_nms_matrix", "gpa_run_boxes", "gpa_scores"]
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpa_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_", "gpf_", "gpv_", "gpm_", "gpl_", "gpg_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the label library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    P, I, D, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    assert list(lib.gpa_descriptors.argtypes) == [P, L, L, P, P, D, I, I, P, P, P]
    assert list(lib.gpa_scores.argtypes) == [P, P, I, I, I, I, I, P, P, P, P, P, P]
    assert list(lib.gpa_run_boxes.argtypes) == [P, P, I, I, I, I, P, P, P, P]
    assert list(lib.gpa_nms_matrix.argtypes) == [P, P, I, I, I, I, P, P] and list(lib.gpa_nms_keep.argtypes) == [P, I, P, P]
    assert lib.gpa_abi_version() >= 1
    header = open(_lib.INCLUDE_DIR + "/gigapose_label.h").read()
    for name, value, mine in (("GPA_Q_BITS", 20, proposals.Q_BITS), ("GPA_MAX_C", 2048, proposals.MAX_C), ("GPA_MAX_K", 64, proposals.MAX_K),
                              ("GPA_MAX_BANK", 1 << 20, proposals.MAX_BANK), ("GPA_MAX_NMS", 8192, proposals.MAX_NMS),
                              ("GPA_MAX_COORD", 1 << 21, ref.MAX_COORD), ("GPA_NON_FINITE", 1, proposals.NON_FINITE),
                              ("GPA_ZERO_NORM", 2, proposals.ZERO_NORM), ("GPA_EMPTY_MASK", 1, proposals.EMPTY_MASK), ("GPA_BAD_MASK", 2, proposals.BAD_MASK)):
        assert f"#define {name} {value}" in header and mine == value, name
    assert (ref.Q_BITS, ref.NON_FINITE, ref.ZERO_NORM, ref.EMPTY_MASK, ref.BAD_MASK) == (20, 1, 2, 1, 2)


def test_label_argument_validation_of_the_library_needs_no_gpu():
    lib = proposals.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(8), ctypes.c_void_p(12)   # `one`: a non-null pointer that is never followed
    err = lib.gpa_last_error

    # Nothing is launched on this machine: the calls that pass are the empty ones
    def desc(cs=257, hs=1, eps=1e-6, B=2, C=384, **p):
        g = {k: p.get(k, one) for k in ("x", "gamma", "beta", "q", "status")}
        return lib.gpa_descriptors(g["x"], cs, hs, g["gamma"], g["beta"], eps, B, C, g["q"], g["status"], null)

    for kw, msg in ((dict(B=-1), b"crops"), (dict(B=2 ** 24 + 1), b"crops"), (dict(C=0), b"channels"), (dict(C=32), b"channels"), (dict(C=100), b"channels"),
                    (dict(C=2112), b"channels"), (dict(cs=0), b"strides"), (dict(hs=-1), b"strides"), (dict(cs=2 ** 40), b"strides"),
                    (dict(eps=-1.0), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps")):
        assert desc(**kw) == -1 and b"gpa_descriptors" in err() and msg in err(), (kw, err())
    for name in ("x", "gamma", "beta", "q", "status"):
        assert desc(**{name: null}) == -1 and b"null" in err(), name
    assert desc(x=ctypes.c_void_p(10)) == -1 and b"aligned" in err() and desc(q=ctypes.c_void_p(10)) == -1 and b"aligned" in err()
    assert desc(B=0, x=null, q=null) == 0 and desc(B=0, C=2048, eps=0.0) == 0 and desc(B=0, C=63) == -1

    def score(P=3, O=2, T=6, C=384, k=5, **p):
        g = {n: p.get(n, one) for n in ("q", "bank", "dot", "obj", "label", "score", "best")}
        return lib.gpa_scores(g["q"], g["bank"], P, O, T, C, k, g["dot"], g["obj"], g["label"], g["score"], g["best"], null)

    for kw, msg in ((dict(O=0), b"bad bank"), (dict(T=0), b"bad bank"), (dict(O=1025, T=1024), b"bad bank"), (dict(O=2 ** 20 + 1, T=1), b"bad bank"),
                    (dict(P=-1), b"proposals"), (dict(P=2 ** 20, O=1024, T=1024), b"proposals"), (dict(C=0), b"channels"), (dict(C=2049), b"channels"),
                    (dict(k=0), b"k ="), (dict(k=65), b"k =")):
        assert score(**kw) == -1 and b"gpa_scores" in err() and msg in err(), (kw, err())
    for name in ("q", "bank", "dot", "label", "score", "best"):
        assert score(**{name: null}) == -1 and b"null" in err(), name
    for name in ("dot", "obj", "score"):
        assert score(**{name: odd}) == -1 and b"8-byte" in err(), name
    assert score(q=ctypes.c_void_p(10)) == -1 and b"4-byte" in err()
    assert score(P=0, q=null, dot=null) == 0 and score(P=0, O=1024, T=1024, C=2048, k=64) == 0 and score(P=0, k=0) == -1

    def boxes(total=10, D=3, H=96, W=128, **p):
        g = {n: p.get(n, one) for n in ("cum", "offsets", "box", "area", "status")}
        return lib.gpa_run_boxes(g["cum"], g["offsets"], total, D, H, W, g["box"], g["area"], g["status"], null)

    for kw in (dict(D=-1), dict(D=65536), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(total=-1)):
        assert boxes(**kw) == -1 and b"gpa_run_boxes" in err() and b"bad sizes" in err(), kw
    for name in ("cum", "offsets", "box", "area", "status"):
        assert boxes(**{name: null}) == -1 and b"null" in err(), name
    assert boxes(area=odd) == -1 and b"aligned" in err()
    assert boxes(D=0, cum=null, area=null) == 0 and boxes(D=0, H=32768, W=65535) == 0

    def matrix(P=5, num=1, den=4, per_label=0, box=one, label=one, sup=one):
        return lib.gpa_nms_matrix(box, label, P, num, den, per_label, sup, null)

    for kw, msg in ((dict(P=-1), b"boxes"), (dict(P=8193), b"boxes"), (dict(num=-1), b"threshold"), (dict(num=5), b"threshold"), (dict(den=0, num=0), b"threshold"),
                    (dict(den=65537), b"threshold")):
        assert matrix(**kw) == -1 and b"gpa_nms_matrix" in err() and msg in err(), kw
    assert matrix(box=null) == -1 and b"null" in err() and matrix(sup=null) == -1 and b"null" in err()
    assert matrix(label=null, per_label=1) == -1 and b"per_label" in err() and matrix(sup=odd) == -1 and b"aligned" in err()
    assert matrix(P=0, box=null, sup=null) == 0 and matrix(P=0, num=65536, den=65536) == 0

    def keep(P=5, sup=one, out=one):
        return lib.gpa_nms_keep(sup, P, out, null)

    for kw in (dict(P=-1), dict(P=8193)):
        assert keep(**kw) == -1 and b"gpa_nms_keep" in err() and b"boxes" in err()
    assert keep(sup=null) == -1 and b"null" in err() and keep(out=null) == -1 and keep(sup=odd) == -1 and b"aligned" in err()
    assert keep(P=0, sup=null, out=null) == 0


def test_label_argument_validation_of_the_python_layer_needs_no_gpu():
    i32 = torch.int32
    x, g = torch.zeros(2, 257, 384), torch.ones(384)
    for kw, match in ((dict(C=100), "channels"), (dict(crop_stride=0), "bad sizes"), (dict(B=3), "leave x"), (dict(gamma=g.double()), "gamma"),
                      (dict(beta=g[:5]), "beta"), (dict(x=x.double()), "float32")):
        a = dict(x=x, crop_stride=257 * 384, channel_stride=1, gamma=g, beta=g, eps=1e-6, B=2, C=384)
        with pytest.raises(ValueError, match=match):
            proposals.descriptors(**dict(a, **kw))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        proposals.descriptors(x, 257 * 384, 1, g, g, 1e-6, 2, 384)
    q, bank = torch.zeros(3, 64, dtype=i32), torch.zeros(2, 6, 64, dtype=i32)
    for a, match in (((q.long(), bank, 5), "q"), ((q, bank.long(), 5), "bank_q"), ((q[:, :32], bank, 5), "q"), ((q, bank[0], 5), "bank_q"),
                     ((q, bank, 0), "bad sizes"), ((q, bank, 65), "bad sizes")):
        with pytest.raises(ValueError, match=match):
            proposals.scores(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        proposals.scores(q, bank, 5)
    box = torch.zeros(4, 4, dtype=i32)
    for a, match in (((box.long(), None, 1, 4), "box"), ((box, None, 5, 4), "threshold"), ((box, None, 1, 0), "threshold"),
                     ((torch.zeros(8193, 4, dtype=i32), None, 1, 4), "limit is 8192"), ((box, torch.zeros(3, dtype=i32), 1, 4, True), "label")):
        with pytest.raises(ValueError, match=match):
            proposals.nms(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        proposals.nms(box, None, 1, 4)
    with pytest.raises(_lib.GigaPoseHipError, match="GPU device"):
        proposals.mask_boxes(np.asarray([4], np.int32), np.asarray([0, 1], np.int32), 2, 2, device="cpu")
    bank = proposals.DescriptorBank.from_arrays(np.zeros((2, 6, 64), np.int32), [1, 2], device="cpu")
    for kw, match in ((dict(top_k=0), "top_k"), (dict(min_score=float("nan")), "NaN"), (dict(nms_iou=(5, 4)), "threshold"), (dict(max_dets=-1), "max_dets")):
        with pytest.raises(ValueError, match=match):
            proposals.ProposalLabeller(None, bank, **kw)
    labeller = proposals.ProposalLabeller(None, bank, device="cpu")
    seg = dict(counts=[6], size=[2, 3])
    with pytest.raises(ValueError, match="2 frames for 1 proposal lists"):
        labeller.label(np.zeros((2, 3, 2, 3), np.uint8), [[]])
    with pytest.raises(ValueError, match="does not match the frame size"):
        labeller.label(np.zeros((1, 3, 4, 4), np.uint8), [[dict(segmentation=seg)]])
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        labeller.label(np.zeros((1, 3, 2, 3), np.uint8), [[dict(segmentation=seg)]])


def test_the_golden_meshes_are_what_label_cases_makes(golden_dir):
    want = cases.golden_meshes()
    with np.load(golden_dir + "/label_meshes.npz") as z:
        assert sorted(z.files) == sorted(want)
        for name in want:
            assert z[name].dtype == want[name].dtype and z[name].tobytes() == want[name].tobytes(), name


def test_descriptor_bank_round_trips_and_refuses_what_is_no_bank(tmp_path):
    rs = np.random.RandomState(6)
    q = cases.quantise(cases.unit_vectors(rs, 3 * 4, 64)).reshape(3, 4, 64)
    bank = proposals.DescriptorBank.from_arrays(q, [7, 2, 30], device="cpu")
    assert len(bank) == 3 and bank.q.shape == (3, 4, 64) and bank.q.dtype == torch.int32
    bank.save(tmp_path / "bank.npz")
    back = proposals.DescriptorBank.load(tmp_path / "bank.npz", device="cpu")
    assert back.labels == [7, 2, 30] and torch.equal(back.q, bank.q) and (back.q.numpy() == q).all()
    with pytest.raises(ValueError, match="needs the ViT"):
        back.add(4, torch.zeros(4, 3, 224, 224))
    for bad_q, labels in ((q.astype(np.int64), [1, 2, 3]), (q, [1, 2]), (q * 2, [1, 2, 3]), (q[0], [1, 2, 3, 4]), (q, [1, 1, 2])):
        with pytest.raises(ValueError, match="DescriptorBank"):
            proposals.DescriptorBank.from_arrays(bad_q, labels, device="cpu")
    np.savez(tmp_path / "other.npz", q=q)
    with pytest.raises(ValueError, match="does not hold a bank"):
        proposals.DescriptorBank.load(tmp_path / "other.npz", device="cpu")
    with pytest.raises(ValueError, match="is empty"):
        proposals.DescriptorBank().q

    class CountingViT:                                            # add() checks the template count before it needs a device
        def cls_descriptors(self, crops):
            return torch.ones(crops.shape[0], 64, dtype=torch.int32), torch.zeros(crops.shape[0], dtype=torch.int32)

    bank = proposals.DescriptorBank(CountingViT())
    bank.add(1, torch.zeros(3, 3, 224, 224)).add(2, dict(rgb=torch.zeros(3, 3, 224, 224)))
    assert bank.labels == [1, 2] and bank.q.shape == (2, 3, 64)
    with pytest.raises(ValueError, match="different template counts"):
        bank.add(3, torch.zeros(4, 3, 224, 224))
    with pytest.raises(ValueError, match="in the bank already"):
        bank.add(2, torch.zeros(3, 3, 224, 224))
    with pytest.raises(ValueError, match=r"expected crops \(T, 3, 224, 224\)"):
        bank.add(5, torch.zeros(3, 3, 98, 98))
