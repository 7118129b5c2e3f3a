"""CPU: the host half of the appearance stage (gigapose_amd/appearance.py, libgigapose_appear.so, include/gigapose_appear.h).

The numpy restatement of the header (gigapose_testing/appear_ref.py) is what the kernels are held to bit for bit
(tests/test_gpu_appear.py); here it is held to readings that cannot share its mistakes: the limbs to the integers they stand for,
the dots to Python integers, the descriptors to fractions.Fraction where every operation is exact, the summation order to a
written-out loop, the occupancy to sets of pixels, the appearance to a brute-force double loop.  Seven subtly wrong scorers fail
these checks.  Beside that: the library against its header, every refusal of the limits message by message, which needs no device,
and the PatchBank."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, appearance, proposals
from gigapose_testing import appear_cases as cases
from gigapose_testing import appear_ref as ref
from gigapose_testing.symbols import exported_symbols


# ---------------------------------------------------------------------------------------------- limbs
def test_limbs_round_trip_on_every_q_and_stay_in_their_ranges():
    q = np.arange(-(1 << 20), (1 << 20) + 1, dtype=np.int32)
    for to_limbs in (ref.q_to_limbs, appearance.q_to_limbs):
        a = to_limbs(q)
        assert a.dtype == np.int8 and a.shape == (3, len(q))
        assert a[:2].min() == -64 and a[:2].max() == 63 and a[2].min() == -64 and a[2].max() == 64
        assert (a[0].astype(np.int64) + 128 * a[1].astype(np.int64) + 16384 * a[2].astype(np.int64) == q).all()
        assert (ref.limbs_to_q(a) == q).all() and (appearance.limbs_to_q(a) == q).all()
    assert ref.q_to_limbs(np.asarray([1 << 20, -(1 << 20), 63, 64, -64, -65])).T.tolist() == [[0, 0, 64], [0, 0, -64], [63, 0, 0], [-64, 1, 0],
                                                                                             [-64, 0, 0], [63, -1, 0]]
    with pytest.raises(ValueError, match="within 2"):
        appearance.q_to_limbs(np.asarray([(1 << 20) + 1]))
    with pytest.raises(ValueError, match="expected int8"):
        appearance.limbs_to_q(np.zeros((2, 4), np.int8))


def test_the_accumulator_bound_holds_at_the_extreme_limbs_and_is_attained():
    C = 2048
    a = cases.extreme_limbs(1, 1, C)
    assert set(np.unique(a[:2]).tolist()) == {-64, 63} and set(np.unique(a[2]).tolist()) == {-64, 64}
    worst = 0
    for i, j in ((0, 0), (0, 1), (1, 1), (2, 3), (5, 0)):
        s = ref.limb_sums(a[:, 0, i], a[:, 0, j])
        worst = max(worst, max(abs(v) for v in s))
        qi, qj = ref.limbs_to_q(a[:, 0, i]).astype(object), ref.limbs_to_q(a[:, 0, j]).astype(object)
        assert ref.combine(s) == int((qi * qj).sum()) and abs(ref.combine(s)) < 1 << 52
    assert worst == 3 * 4096 * C == 3 << 23 < 1 << 31          # patch 0 against itself: the bound of the header, attained


# ---------------------------------------------------------------------------------------------- restatement against exact arithmetic
def test_restated_dots_equal_python_integer_dots():
    for C, seed in ((64, 1), (128, 2)):
        case = cases.planted_pairs(seed, C)
        got = ref.dots(case["qa"][:, 0], case["ta"][:, 0])
        q, t = ref.limbs_to_q(case["qa"][:, 0]).tolist(), ref.limbs_to_q(case["ta"][:, 0]).tolist()
        for i in (0, 7, 100, 255):
            assert got[i].tolist() == [sum(x * y for x, y in zip(q[i], t[j])) for j in range(256)]
    a = cases.extreme_limbs(3, 1, 2048)
    got = ref.dots(a[:, 0], a[:, 0])
    q = ref.limbs_to_q(a[:, 0]).tolist()
    assert got.dtype == np.int64 and got[0, 0] == sum(x * x for x in q[0]) and got[1, 0] == sum(x * y for x, y in zip(q[1], q[0]))
    assert got[3, 200] == sum(x * y for x, y in zip(q[3], q[200]))


def test_restated_descriptors_equal_rational_arithmetic_where_every_operation_is_exact():
    """x = +-1 in equal numbers IN EVERY CHAIN, gamma = 1, beta = 0, eps = 0: mean 0, variance 1, norm sqrt(C) = 8, 16, 32."""
    for C in (64, 256, 1024):
        rs = np.random.RandomState(C)
        x = np.empty(C, np.float32)
        for j in range(4):
            x[j::4] = np.where(rs.permutation(C // 4) % 2 == 0, 1.0, -1.0)
        xs = [Fraction(float(v)) for v in x]
        mean = sum(xs) / C
        var = sum((v - mean) ** 2 for v in xs) / C
        assert mean == 0 and var == 1
        norm = Fraction(int(np.sqrt(C)))
        want = [int((v - mean) / norm * (1 << 20)) for v in xs]                                  # exact: 2^20 / 2^k
        q, status = ref.quantised(x[None], np.ones(C, np.float32), np.zeros(C, np.float32), 0.0)
        assert status[0] == 0 and q[0].tolist() == want
        a, st = ref.patch_descriptors(np.broadcast_to(x, (1, 256, C)), np.ones(C, np.float32), np.zeros(C, np.float32), 0.0)
        assert a.shape == (3, 1, 256, C) and a.dtype == np.int8 and st.shape == (1, 256) and (ref.limbs_to_q(a)[0] == q[0]).all()
    gamma, beta = cases.label_cases.norm_parameters(2, 64, zero_beta=True)
    x, kinds = cases.patch_tokens(3, 1, 64)
    a, status = ref.patch_descriptors(x, gamma, beta, cases.EPS)
    for n, kind in enumerate(kinds[:10]):
        want = {"constant": ref.ZERO_NORM, "nan": ref.NON_FINITE, "inf": ref.NON_FINITE}.get(kind, 0)
        assert status[0, n] == want and (a[:, 0, n] != 0).any() == (want == 0), kind


def test_restated_sum_takes_the_headers_four_chains_not_numpys_pairwise_sum():
    rs = np.random.RandomState(5)
    v = rs.standard_normal((40, 768)) * 10.0 ** rs.uniform(-3, 3, (40, 768))
    got = ref.chain_sum(v)
    for b in range(40):
        S = [0.0, 0.0, 0.0, 0.0]
        for c in range(768):
            S[c % 4] = S[c % 4] + float(v[b, c])
        assert got[b] == (S[0] + S[1]) + (S[2] + S[3])
    assert (got != v.sum(axis=1)).any()
    # a case where the two differ: chain 0 meets 1, 2^-53, 0, 2^-53 in that order and loses both small terms (half an ulp each, ties to
    # even); numpy's sum keeps elements 4 and 12 in an accumulator of their own, where they add up to a whole ulp
    w = np.zeros(128)
    w[0], w[4], w[12] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ref.chain_sum(w[None])[0] == ((1.0 + 2.0 ** -53) + 2.0 ** -53) == 1.0
    assert w.sum() == 1.0 + 2.0 ** -52 != ref.chain_sum(w[None])[0]


# ---------------------------------------------------------------------------------------------- occupancy
def test_occupancy_equals_a_pixel_set_reading():
    mask, planted = cases.planted_masks(3, seed=4)
    assert np.isnan(mask).any() and (mask == 0.5).any()
    for num, den in ((1, 2), (0, 1), (1, 1), (97, 196)):
        valid, count, sets = ref.patch_valid(mask, num, den)
        assert valid.dtype == np.uint8 and count.dtype == np.int32 and sets.dtype == np.uint8
        for b in range(3):
            pixels = {(y, x) for y, x in zip(*np.nonzero(np.nan_to_num(mask[b], nan=0.0) > 0.5))}
            per_patch = [0] * 256
            for y, x in pixels:
                per_patch[16 * (y // 14) + x // 14] += 1
            assert sets[b].tolist() == per_patch
            assert valid[b].tolist() == [int(Fraction(k, 196) > Fraction(num, den)) for k in per_patch] and count[b] == valid[b].sum()
        for (b, patch), k in planted.items():
            assert sets[b, patch] == k
            if (num, den) == (1, 2):
                assert valid[b, patch] == (k >= 99)                                              # 98 of 196 is not MORE than a half
            if (num, den) == (0, 1):
                assert valid[b, patch] == (k >= 1)
            if (num, den) == (1, 1):
                assert valid[b, patch] == 0                                                      # more than all: never
    assert {97, 98, 99, 0, 196} <= set(planted.values())


# ---------------------------------------------------------------------------------------------- appearance
def brute_force(qa, q_valid, ta, t_valid, q, t):
    """One pair in Python integers: -> (sum, n, best list, arg list)."""
    Q, Tm = ref.limbs_to_q(qa[:, q]).tolist(), ref.limbs_to_q(ta[:, t]).tolist()
    best, arg = [0] * 256, [-1] * 256
    total = n = 0
    for i in range(256):
        if not q_valid[q, i]:
            continue
        top = None
        for j in range(256):
            if not t_valid[t, j]:
                continue
            d = sum(x * y for x, y in zip(Q[i], Tm[j]))
            if top is None or d > top:
                top, arg[i] = d, j
        best[i] = top
        total, n = total + top, n + 1
    return total, n, best, arg


def plants_hold(case, out, p=0):
    """The planted answers of appear_cases.planted_pairs in pair p = (crop 0, row 0)."""
    i = case["plants"]
    arg, best = out["arg"][p], out["best"][p]
    ok = [int(arg[i[k]]) for k in range(4)] == list(cases.PLANTED_MAX_AT)
    ok &= arg[i[4]] == cases.TIE_TILES[0] and arg[i[5]] == cases.TIE_LANES[0]                    # of equal maxima the first j
    ok &= arg[i[6]] != cases.INVALID_WINNER
    q = ref.limbs_to_q(case["qa"][:, 0]).astype(np.int64)
    ok &= all(best[i[k]] == (q[i[k]] ** 2).sum() for k in range(6)) and best[i[6]] < (q[i[6]] ** 2).sum()
    return bool(ok)


def test_appearance_equals_a_brute_force_double_loop():
    case = cases.planted_pairs(11, 64)
    qi, ti = cases.all_pairs_with_bad(4, 4)
    out = ref.appearance(case["qa"], case["q_valid"], case["ta"], case["t_valid"], qi, ti)
    assert plants_hold(case, out)
    for p, (q, t) in enumerate(zip(qi.tolist(), ti.tolist())):
        if not (0 <= q < 4 and 0 <= t < 4):
            assert out["status"][p] == ref.BAD_INDEX
            want = (0, 0, [0] * 256, [-1] * 256)
        else:
            flag = (ref.NO_QUERY_PATCH if q == 2 else 0) | (ref.NO_TEMPLATE_PATCH if t == 2 else 0)
            assert out["status"][p] == flag
            want = (0, 0, [0] * 256, [-1] * 256) if flag else brute_force(case["qa"], case["q_valid"], case["ta"], case["t_valid"], q, t)
        assert (int(out["sum"][p]), int(out["n"][p]), out["best"][p].tolist(), out["arg"][p].tolist()) == want, (p, q, t)
    p33 = int(np.flatnonzero((qi == 3) & (ti == 3))[0])
    assert (out["best"][p33] < 0).all() and out["n"][p33] == 256                                  # a crop against its negative
    p11 = int(np.flatnonzero((qi == 1) & (ti == 1))[0])
    assert out["n"][p11] == 1 and out["arg"][p11, cases.ONE_QUERY] == cases.ONE_TEMPLATE
    score = ref.float_appearance(out["sum"], out["n"])
    assert score[p33] < 0 and score[int(np.flatnonzero(out["status"] != 0)[0])] == 0.0
    assert (appearance.float_appearance(out["sum"], out["n"]) == score).all()
    assert (appearance.float_appearance(torch.from_numpy(out["sum"]), torch.from_numpy(out["n"])).numpy() == score).all()


# ---------------------------------------------------------------------------------------------- the wrong versions
def checks_pass(variant):
    """The checks above in small: True when `variant` passes all of them."""
    ok = True
    case = cases.planted_pairs(11, 64)
    out = ref.appearance(case["qa"], case["q_valid"], case["ta"], case["t_valid"], [0, 3, 0], [0, 3, 1], variant)
    ok &= plants_hold(case, out)
    for p, (q, t) in enumerate(((0, 0), (3, 3), (0, 1))):
        want = brute_force(case["qa"], case["q_valid"], case["ta"], case["t_valid"], q, t)
        ok &= (int(out["sum"][p]), int(out["n"][p]), out["arg"][p].tolist()) == (want[0], want[1], want[3])
    # quantisation: a component at 2^-20 * (k + 0.75) rounds up; and the limbs of the extremes respect the accumulator bound
    C = 64
    x = np.zeros((1, C), np.float32)
    x[0, 0], x[0, 1], x[0, 2] = 2.0, -1.0, -1.0                                                  # (2, -1, -1) / sqrt(6): 2^21 / sqrt(6) = 856158.72..
    q, _ = ref.quantised(x, np.ones(C, np.float32), np.zeros(C, np.float32), 0.0, variant)
    ok &= q[0, :3].tolist() == [856159, -428079, -428079]
    a = ref.q_to_limbs(np.full((2048,), 16383), variant)
    ok &= max(abs(v) for v in ref.limb_sums(a, a)) <= 3 << 23 and int(np.abs(a[:2]).max()) <= 64
    return bool(ok)


def test_the_checks_hold_for_the_restatement():
    assert checks_pass(None)


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_checks_reject_wrong_versions(variant):
    assert len(ref.VARIANTS) == 7 and not checks_pass(variant)


# ---------------------------------------------------------------------------------------------- the library and its header
def test_appear_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_appear.so", "gpp")      # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_appear.h" and side.path == appearance.APPEAR_LIB_PATH
    assert sorted(protos) == ["gpp_abi_version", "gpp_appearance", "gpp_last_error", "gpp_patch_descriptors", "gpp_patch_valid"]
    assert all(n.startswith("gpp_") for n in protos)
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpp_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_", "gpf_", "gpv_", "gpm_", "gpl_", "gpg_", "gpa_", "gpc_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the appearance library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    P, I, D, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    assert list(lib.gpp_patch_descriptors.argtypes) == [P, L, L, L, P, P, D, I, I, P, P, P]
    assert list(lib.gpp_patch_valid.argtypes) == [P, I, I, I, P, P, P, P]
    assert list(lib.gpp_appearance.argtypes) == [P, P, I, P, P, I, I, P, P, I, P, P, P, P, P, P]
    assert lib.gpp_abi_version() >= 1
    header = open(_lib.INCLUDE_DIR + "/gigapose_appear.h").read()
    for name, value, mine in (("GPP_PATCHES", 256, appearance.PATCHES), ("GPP_CELL", 14, appearance.CELL), ("GPP_Q_BITS", 20, appearance.Q_BITS),
                              ("GPP_MAX_C", 2048, appearance.MAX_C), ("GPP_MAX_ROWS", 1 << 20, appearance.MAX_ROWS),
                              ("GPP_MAX_PAIRS", 65535, appearance.MAX_PAIRS), ("GPP_NON_FINITE", 1, appearance.NON_FINITE),
                              ("GPP_ZERO_NORM", 2, appearance.ZERO_NORM), ("GPP_BAD_INDEX", 1, appearance.BAD_INDEX),
                              ("GPP_NO_QUERY_PATCH", 2, appearance.NO_QUERY_PATCH), ("GPP_NO_TEMPLATE_PATCH", 4, appearance.NO_TEMPLATE_PATCH)):
        assert f"#define {name} {value}" in header and mine == value, name
    assert (ref.PATCHES, ref.CELL, ref.Q_BITS, ref.NON_FINITE, ref.ZERO_NORM, ref.BAD_INDEX, ref.NO_QUERY_PATCH, ref.NO_TEMPLATE_PATCH) == (256, 14, 20, 1, 2, 1, 2, 4)
    assert appearance.Q_BITS == proposals.Q_BITS and "3 * 4096 * 2048 = 3 * 2^23" in header      # the bound is stated


def test_appear_argument_validation_of_the_library_needs_no_gpu():
    lib = appearance.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68)   # `one`: a non-null pointer that is never followed
    err = lib.gpp_last_error

    # Nothing is launched on this machine: the calls that pass are the empty ones
    def desc(cs=257, ts=1, hs=65792, eps=1e-6, B=2, C=384, **p):
        g = {k: p.get(k, one) for k in ("x", "gamma", "beta", "a", "status")}
        return lib.gpp_patch_descriptors(g["x"], cs, ts, hs, g["gamma"], g["beta"], eps, B, C, g["a"], g["status"], null)

    for kw, msg in ((dict(B=-1), b"crops"), (dict(B=2 ** 20 + 1), b"crops"), (dict(C=0), b"channels"), (dict(C=32), b"channels"), (dict(C=100), b"channels"),
                    (dict(C=2112), b"channels"), (dict(cs=0), b"strides"), (dict(ts=0), b"strides"), (dict(hs=-1), b"strides"), (dict(ts=2 ** 40), b"strides"),
                    (dict(eps=-1.0), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps")):
        assert desc(**kw) == -1 and b"gpp_patch_descriptors" in err() and msg in err(), (kw, err())
    for name in ("x", "gamma", "beta", "a", "status"):
        assert desc(**{name: null}) == -1 and b"null" in err(), name
    assert desc(x=ctypes.c_void_p(10)) == -1 and b"aligned" in err() and desc(a=odd) == -1 and b"aligned" in err()
    assert desc(B=0, x=null, a=null) == 0 and desc(B=0, C=2048, eps=0.0) == 0 and desc(B=0, C=63) == -1

    def occupancy(B=2, num=1, den=2, mask=one, valid=one, count=one, pixels=one):
        return lib.gpp_patch_valid(mask, B, num, den, valid, count, pixels, null)

    for kw, msg in ((dict(B=-1), b"crops"), (dict(B=2 ** 20 + 1), b"crops"), (dict(num=-1), b"threshold"), (dict(num=3), b"threshold"),
                    (dict(den=0, num=0), b"threshold"), (dict(den=65537), b"threshold")):
        assert occupancy(**kw) == -1 and b"gpp_patch_valid" in err() and msg in err(), kw
    for name in ("mask", "valid", "count"):
        assert occupancy(**{name: null}) == -1 and b"null" in err(), name
    assert occupancy(mask=ctypes.c_void_p(10)) == -1 and b"aligned" in err()
    assert occupancy(B=0, mask=null, valid=null, count=null, pixels=null) == 0 and occupancy(B=0, num=65536, den=65536) == 0

    def score(Bq=3, R=4, C=384, P=5, **p):
        g = {n: p.get(n, one) for n in ("qa", "q_valid", "ta", "t_valid", "qi", "ti", "sum", "n", "status", "best", "arg")}
        return lib.gpp_appearance(g["qa"], g["q_valid"], Bq, g["ta"], g["t_valid"], R, C, g["qi"], g["ti"], P, g["sum"], g["n"], g["status"], g["best"],
                                  g["arg"], null)

    for kw, msg in ((dict(P=-1), b"pairs"), (dict(P=65536), b"pairs"), (dict(Bq=0), b"bad sizes"), (dict(R=0), b"bad sizes"), (dict(Bq=2 ** 20 + 1), b"bad sizes"),
                    (dict(R=2 ** 20 + 1), b"bad sizes"), (dict(C=0), b"channels"), (dict(C=96), b"channels"), (dict(C=2112), b"channels")):
        assert score(**kw) == -1 and b"gpp_appearance" in err() and msg in err(), (kw, err())
    for name in ("qa", "q_valid", "ta", "t_valid", "qi", "ti", "sum", "n", "status"):
        assert score(**{name: null}) == -1 and b"null" in err(), name
    for name in ("qa", "ta"):
        assert score(**{name: odd}) == -1 and b"16-byte" in err(), name
    for name in ("sum", "best"):
        assert score(**{name: odd}) == -1 and b"8-byte" in err(), name
    assert score(P=0, qa=null, sum=null, best=null, arg=null) == 0 and score(P=0, Bq=2 ** 20, R=2 ** 20, C=2048) == 0 and score(P=0, C=32) == -1


def test_appear_argument_validation_of_the_python_layer_needs_no_gpu():
    x, g = torch.zeros(2, 257, 128), torch.ones(128)
    good = dict(x=x, crop_stride=257 * 128, token_stride=128, channel_stride=1, gamma=g, beta=g, eps=1e-6, B=2, C=128, offset=128)
    for kw, match in ((dict(C=100), "channels"), (dict(crop_stride=0), "bad sizes"), (dict(token_stride=0), "bad sizes"), (dict(offset=-1), "bad sizes"),
                      (dict(B=3), "leave x"), (dict(offset=129), "leave x"), (dict(gamma=g.double()), "gamma"), (dict(beta=g[:5]), "beta"),
                      (dict(x=x.double()), "float32")):
        with pytest.raises(ValueError, match=match):
            appearance.patch_descriptors(**dict(good, **kw))
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        appearance.patch_descriptors(**good)
    mask = torch.zeros(2, 224, 224)
    for a, match in (((mask.double(),), "mask"), ((mask[:, :100],), "mask"), ((mask, 3, 2), "threshold"), ((mask, 1, 0), "threshold"), ((mask, -1, 2), "threshold")):
        with pytest.raises(ValueError, match=match):
            appearance.patch_valid(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        appearance.patch_valid(mask)
    i8, u8, i32 = torch.int8, torch.uint8, torch.int32
    qa, qv, ta, tv = torch.zeros(3, 2, 256, 64, dtype=i8), torch.ones(2, 256, dtype=u8), torch.zeros(3, 4, 256, 64, dtype=i8), torch.ones(4, 256, dtype=u8)
    qi, ti = torch.zeros(5, dtype=i32), torch.zeros(5, dtype=i32)
    for a, match in (((qa.int(), qv, ta, tv, qi, ti), "qa"), ((qa[0], qv, ta, tv, qi, ti), "qa must be"), ((qa, qv, ta[:, :, :, :32], tv, qi, ti), "ta"),
                     ((qa, qv[:1], ta, tv, qi, ti), "q_valid"), ((qa, qv, ta, tv.bool(), qi, ti), "t_valid"), ((qa, qv, ta, tv, qi.long(), ti), "qi"),
                     ((qa, qv, ta, tv, qi, ti[:4]), "ti"), ((qa[:, :0], qv[:0], ta, tv, qi, ti), "bad sizes"),
                     ((torch.zeros(3, 2, 256, 96, dtype=i8), qv, torch.zeros(3, 4, 256, 96, dtype=i8), tv, qi, ti), "bad sizes"),
                     ((qa, qv, ta, tv, qi, ti, ("dot",)), "want takes")):
        with pytest.raises(ValueError, match=match):
            appearance.appearance(*a)
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        appearance.appearance(qa, qv, ta, tv, qi, ti)


# ---------------------------------------------------------------------------------------------- the bank
def small_bank_arrays(O=3, T=2, C=64, seed=6):
    rs = np.random.RandomState(seed)
    a = ref.q_to_limbs(cases.quantised_units(rs, (O, T, 256), C))
    valid = (rs.uniform(size=(O, T, 256)) < 0.5).astype(np.uint8)
    valid[..., 0] = 1
    return a, valid


def test_patch_bank_round_trips_and_refuses_what_is_no_bank(tmp_path):
    a, valid = small_bank_arrays()
    bank = appearance.PatchBank.from_arrays(a, valid, [7, 2, 30], device="cpu")
    assert len(bank) == 3 and bank.templates == 2 and bank.a.shape == (3, 6, 256, 64) and bank.a.dtype == torch.int8
    assert bank.valid.shape == (6, 256) and bank.valid.dtype == torch.uint8
    assert (bank.a.numpy().reshape(a.shape) == a).all() and (bank.valid.numpy().reshape(valid.shape) == valid).all()
    bank.save(tmp_path / "patches.npz")
    back = appearance.PatchBank.load(tmp_path / "patches.npz", device="cpu")
    assert back.labels == [7, 2, 30] and torch.equal(back.a, bank.a) and torch.equal(back.valid, bank.valid)
    with pytest.raises(ValueError, match="needs the ViT"):
        back.add(4, torch.zeros(2, 3, 224, 224), torch.zeros(2, 224, 224))
    empty = valid.copy()
    empty[1, 1] = 0
    big = a.copy()
    big[0, 0, 0, 0, 0] = 64                                                                      # a0 = 64 leaves [-64, 63]
    for bad in ((a.astype(np.int16), valid, [1, 2, 3]), (a, valid.astype(bool), [1, 2, 3]), (a, valid, [1, 2]), (a[:2], valid, [1, 2, 3]),
                (a, valid[:, :1], [1, 2, 3]), (a, valid, [1, 1, 2]), (big, valid, [1, 2, 3]), (a[..., :32], valid, [1, 2, 3])):
        with pytest.raises(ValueError, match="PatchBank"):
            appearance.PatchBank.from_arrays(*bad, device="cpu")
    with pytest.raises(ValueError, match="object 2: template 1 has no valid patch"):
        appearance.PatchBank.from_arrays(a, empty, [1, 2, 3], device="cpu")
    np.savez(tmp_path / "other.npz", a=a)
    with pytest.raises(ValueError, match="does not hold a patch bank"):
        appearance.PatchBank.load(tmp_path / "other.npz", device="cpu")
    with pytest.raises(ValueError, match="is empty"):
        appearance.PatchBank().a
    with pytest.raises(ValueError, match="threshold"):
        appearance.PatchBank(occupancy=(3, 2))


def test_patch_bank_add_checks_counts_and_names_a_template_without_patches():
    class CountingViT:                                            # add() checks the template count before it needs a device
        def cls_and_patch_descriptors(self, crops, masks, occupancy=(1, 2)):
            n = crops.shape[0]
            count = (masks.flatten(1) > 0.5).sum(dim=1).clamp(max=1).int()                       # a template with an all-zero mask has no patch
            return dict(a=torch.ones(3, n, 256, 64, dtype=torch.int8), valid=torch.ones(n, 256, dtype=torch.uint8) * count[:, None].to(torch.uint8), count=count)

    crops, masks = torch.zeros(3, 3, 224, 224), torch.ones(3, 224, 224)
    bank = appearance.PatchBank(CountingViT())
    bank.add(1, crops, masks).add(2, dict(rgb=crops, mask=masks))
    assert bank.labels == [1, 2] and bank.a.shape == (3, 6, 256, 64) and bank.valid.shape == (6, 256) and bank.templates == 3
    bank.add(9, dict(rgb=crops, mask=masks))                       # after the joined view was taken: the bank grows
    assert bank.a.shape == (3, 9, 256, 64) and bank.labels == [1, 2, 9]
    with pytest.raises(ValueError, match="different template counts"):
        bank.add(3, torch.zeros(4, 3, 224, 224), torch.ones(4, 224, 224))
    with pytest.raises(ValueError, match="in the bank already"):
        bank.add(2, crops, masks)
    with pytest.raises(ValueError, match=r"expected crops \(T, 3, 224, 224\)"):
        bank.add(5, torch.zeros(3, 3, 98, 98), masks)
    with pytest.raises(ValueError, match=r"expected masks \(3, 224, 224\)"):
        bank.add(5, crops, masks[:2])
    holed = masks.clone()
    holed[1] = 0
    with pytest.raises(ValueError, match="object 5: template 1 has no valid patch"):
        bank.add(5, crops, holed)
    assert bank.labels == [1, 2, 9]


def test_the_labeller_refuses_a_patch_bank_with_other_labels_and_ignores_none():
    a, valid = small_bank_arrays(O=2, T=6)
    dbank = proposals.DescriptorBank.from_arrays(np.zeros((2, 6, 64), np.int32), [1, 2], device="cpu")
    with pytest.raises(ValueError, match="the same labels in the same order"):
        proposals.ProposalLabeller(None, dbank, appearance=appearance.PatchBank.from_arrays(a, valid, [2, 1], device="cpu"))
    labeller = proposals.ProposalLabeller(None, dbank, appearance=appearance.PatchBank.from_arrays(a, valid, [1, 2], device="cpu"), device="cpu")
    assert labeller.appearance.labels == [1, 2] and proposals.ProposalLabeller(None, dbank).appearance is None
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        labeller.label(np.zeros((1, 3, 2, 3), np.uint8), [[dict(segmentation=dict(counts=[6], size=[2, 3]))]])
