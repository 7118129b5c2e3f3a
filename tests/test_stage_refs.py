"""CPU: the float64 references and input builders of the split path's stage tests (gigapose_testing/stage_refs.py) against torch's
own float64 operators, and every "reference alone" condition those tests rely on -- so that a failure of a GPU stage test is a
finding about a kernel, not about its yardstick.  No GPU, no HIP library."""
import numpy as np
import pytest
import torch

from gigapose_testing import stage_refs as sr

F = torch.nn.functional


# ---------------------------------------------------------------------------------------------------------------- planes
@pytest.mark.parametrize("scale", [8.0, 64.0, 0.25, 1.0, 3.3])
def test_host_split_reconstructs_to_22_bits_and_is_well_formed(scale):
    x = torch.from_numpy(sr.split_values_case(100003, 5))
    hi, lo = sr.split_planes_host(x, scale)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    v = (x * torch.tensor(scale, dtype=torch.float32)).double()            # the f32 product the planes split
    fits = v.abs() < 65504.0                                               # 8000 x 64 leaves f16: hi = inf there, on the device too
    assert int(fits.sum()) > 90000 and bool(torch.isinf(hi[~fits].float()).all())
    v, hi, lo = v[fits], hi[fits], lo[fits]
    back = hi.double() + lo.double()
    # 22 bits of v, down to the f16 subnormal floor of the lo plane (2^-25 absolute)
    assert bool(((back - v).abs() <= sr.PLANE_BITS * v.abs() + 2.0 ** -25).all())
    assert sr.planes_well_formed(hi, lo)
    big = v.abs() >= 0.25                  # lo = f16(v - hi) is a normal f16 or an exact subnormal from here up: the pure relative statement
    assert int(big.sum()) > 1000 and float(((back - v).abs() / v.abs())[big].max()) <= sr.PLANE_BITS


def test_host_split_on_hand_computed_values():
    hi, lo = sr.split_planes_host(torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, 0.0, -0.0, 1.0 + 2.0 ** -20]), 1.0)
    # ties go to even: 1 + 2^-11 -> 1 (lo = +2^-11), 1 + 3 * 2^-11 -> 1 + 2^-9 (lo = -2^-11)
    assert hi.tolist() == [1.0, 1.0 + 2.0 ** -9, 0.0, -0.0, 1.0]
    assert lo.tolist() == [2.0 ** -11, -2.0 ** -11, 0.0, 0.0, 2.0 ** -20]
    assert torch.signbit(hi[3]) and not torch.signbit(hi[2])
    # x 3.3 is not exact: the planes split the ROUNDED f32 product, not the exact one
    x = torch.tensor([0.7], dtype=torch.float32)
    hi, lo = sr.split_planes_host(x, 3.3)
    v = np.float32(0.7) * np.float32(3.3)
    assert float(hi) == float(np.float16(v)) and float(lo) == float(np.float16(v - np.float32(np.float16(v))))


def test_split_values_case_holds_what_it_is_named_after():
    x = sr.split_values_case(257, 1)
    assert x.dtype == np.float32 and x.shape == (257,)
    a = np.abs(x[x != 0])
    assert a.min() <= 1e-29 and a.max() >= 7999.0 and a.max() <= 8000.0
    assert (x == 0).sum() >= 2 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    hi, lo = sr.split_planes_host(torch.from_numpy(x), 1.0)
    nz = x != 0
    assert int(((lo == 0) & torch.from_numpy(nz) & (hi != 0)).sum()) >= 4                      # exact f16 values
    assert int(((lo != 0) & (lo.double().abs() < 2.0 ** -14)).sum()) >= 3                     # f16-subnormal lows
    assert int((lo.double().abs() == 0.5 * sr.f16_ulp(hi)).sum()) >= 3                        # halfway cases
    assert sr.split_values_case(1, 3).shape == (1,)


def test_f16_ulp():
    h = torch.tensor([1.0, 1.5, 2.0, 1000.0, 2.0 ** -14, 2.0 ** -15, 0.0, -3.0, 65504.0], dtype=torch.float16)
    assert sr.f16_ulp(h).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9, 32.0]
    assert not sr.planes_well_formed(torch.tensor([1.0], dtype=torch.float16), torch.tensor([2.0 ** -10], dtype=torch.float16))
    assert not sr.planes_well_formed(torch.tensor([float("inf")], dtype=torch.float16), torch.tensor([0.0], dtype=torch.float16))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("C,Mpad", [(384, 1024), (1024, 2304), (1280, 1024), (128, 512)])
def test_layernorm_f64_equals_torch_and_the_classes_are_what_they_say(C, Mpad):
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, 11)
    y, xhat = sr.layernorm_f64(x, gamma, beta, 1e-6)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-6)
    assert float((y - ref).abs().max()) < 1e-12
    # the classes
    names = sr.LN_CLASSES
    assert set(cls.tolist()) == set(range(5))
    plain, massive, offset, const, pad = (x[cls == i].double() for i in range(5))
    assert abs(float(plain.mean())) < 0.1 and 0.3 < float(plain.std(dim=1).min()) and float(plain.std(dim=1).max()) < 3.6
    assert float(massive[:, 7].min()) > 235 and float(massive[:, C - 3].max()) < -165
    assert float(offset.mean(dim=1).min()) > 49 and float((offset.mean(dim=1) / offset.std(dim=1)).min()) > 10   # mean >> spread
    assert bool((const == 3.0).all()) and bool((pad == 0.0).all())
    # positions: first / last columns of 16-, 32- and 64-token blocks and the end of the buffer carry special tokens
    cols = sr.layernorm_class_columns(Mpad)
    for name in ("massive", "offset", "constant"):
        assert all(int(cls[c]) == names.index(name) for c in cols[name]) and Mpad - 4 <= max(cols[name])
    assert {c % 16 for cc in cols.values() for c in cc} >= {0, 15} and {c % 64 for cc in cols.values() for c in cc} >= {0, 63, 31, 32}
    assert int(cls[Mpad - 1]) == 4
    # constant and pad tokens: x - mean is exactly 0, y = beta exactly; the guard is far away (max |8 y| a few hundred)
    assert bool((y[(cls == 3) | (cls == 4)] == beta.double()).all())
    assert float((8 * y).abs().max()) < 1000.0
    # the reference alone (ATen's f32 LayerNorm on the CPU) per class: f32-class figures, the offset class an order above the others
    e = sr.per_class_max(sr.layernorm_error(F.layer_norm(x, (C,), gamma, beta, 1e-6), y, xhat, gamma, beta), cls)
    print(f"C={C} Mpad={Mpad}: f32 CPU LayerNorm vs float64 per class: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["plain"] < 5e-7 and e["massive"] < 5e-7 and 1e-6 < e["offset"] < 3e-5 and e["constant"] == 0 and e["pad"] == 0
    # ... and the numpy f32 model of the kernels' own summation orders (16 / 32 interleaved partial sums of the register kernels, 16
    # contiguous slices of the three-pass kernel) is an f32 LayerNorm of the same class: exact where the sums are exact, a few ulp elsewhere
    for slices, contiguous in ((16, False), (32, False), (16, True)):
        if C % (8 * slices):
            continue
        m = sr.per_class_max(sr.layernorm_error(torch.from_numpy(sr.layernorm_partial_sums_f32(x.numpy(), gamma.numpy(), beta.numpy(), 1e-6, slices,
                                                                                                  contiguous)), y, xhat, gamma, beta), cls)
        print(f"   model with {slices} {'contiguous' if contiguous else 'interleaved'} partial sums: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
        assert m["plain"] < 5e-7 and m["massive"] < 5e-7 and 1e-6 < m["offset"] < 3e-5 and m["constant"] == 0 and m["pad"] == 0


def test_layernorm_reference_notices_a_wrong_variance():
    """The measure separates the biased from the unbiased variance (1 / C vs 1 / (C - 1): a relative 1.3e-3 at C = 384)."""
    C = 384
    x, cls, gamma, beta = sr.layernorm_case(C, 1024, 12)
    y, xhat = sr.layernorm_f64(x, gamma, beta, 1e-6)
    xd = x.double()
    wrong = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=True, keepdim=True) + 1e-6) * gamma.double() + beta.double()
    e = sr.per_class_max(sr.layernorm_error(wrong, y, xhat, gamma, beta), cls)
    assert e["plain"] > 1e-4 and e["massive"] > 1e-4 and e["offset"] > 1e-4


# ---------------------------------------------------------------------------------------------------------------- the split stem
@pytest.mark.parametrize("S,Cout,B", [(32, 16, 2), (64, 128, 1), (18, 8, 3)])
def test_framed_stem_reference_equals_conv2d(S, Cout, B):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, 3, S, S, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 3, 7, 7, generator=g, dtype=torch.float64)
    got = sr.stem_conv_framed_f64(sr.frame_image(x), sr.pack_stem_weights(w))
    ref = F.conv2d(x, w, stride=2, padding=3)
    assert got.shape == ref.shape == (B, Cout, S // 2, S // 2)
    assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    wk = sr.pack_stem_weights(w).reshape(Cout, 7, 8, 4)
    assert bool((wk[:, :, 7] == 0).all()) and bool((wk[..., 3] == 0).all())
    assert wk[3, 2, 5, 1] == w[3, 1, 2, 5]                       # k = dy * 32 + dx * 4 + ci
    fr = sr.frame_image(x)
    assert fr.shape == (B, S + 6, S + 8, 4) and bool((fr[:, :3] == 0).all()) and bool((fr[:, S + 3:] == 0).all())
    assert bool((fr[:, :, :3] == 0).all()) and bool((fr[:, :, S + 3:] == 0).all()) and bool((fr[..., 3] == 0).all())
    a, b = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    full = sr.bn_relu_f64(got, a, b, True)
    assert float((full - torch.relu(ref * a.double()[None, :, None, None] + b.double()[None, :, None, None])).abs().max()) < 1e-10
    assert sr.bn_relu_f64(got, None, None, False) is got


def test_framed_stem_reference_notices_a_shifted_frame():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3, 32, 32, generator=g, dtype=torch.float64)
    w = torch.randn(8, 3, 7, 7, generator=g, dtype=torch.float64)
    fr = torch.roll(sr.frame_image(x), 1, dims=2)               # image one column to the right
    assert float((sr.stem_conv_framed_f64(fr, sr.pack_stem_weights(w)) - F.conv2d(x, w, stride=2, padding=3)).abs().max()) > 0.1


def test_resize_reference_identity_and_f32_error():
    g = torch.Generator().manual_seed(2)
    for (IH, IW, S) in [(224, 224, 256), (200, 312, 256), (256, 256, 256), (224, 224, 32), (37, 53, 64)]:
        x = torch.randn(3, 3, IH, IW, generator=g)
        r64 = sr.resize_f64(x, S)
        r32 = F.interpolate(x, (S, S), mode="bilinear", align_corners=True)
        e = float((r32.double() - r64).abs().max())
        # f32 places a sample with the rounded ratio (IH - 1) / (S - 1): up to 1e-5 of a pixel off at the far border, times the slope of noise
        assert r64.shape == (3, 3, S, S) and e < 2e-4
        if IH == S and IW == S:
            assert torch.equal(r64, x.double()) and e == 0.0


# ---------------------------------------------------------------------------------------------------------------- IST regressor
def _ist(seed):
    from test_oracle_pose_ist import build_ist, mlp_weights

    net = build_ist(seed)
    return net, mlp_weights(net)


def test_ist_regressor_f64_equals_the_module_in_double():
    net, w = _ist(101)
    feats = torch.randn(300, 512, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    sc, cs = sr.ist_regressor_f64(feats, w)
    reg = net.regressor.double()
    with torch.no_grad():
        rsc, rcs = reg.scale_predictor(feats)[:, 0], reg.inplane_predictor(feats)
    assert float((sc - rsc).abs().max()) < 1e-12 and float((cs - rcs).abs().max()) < 1e-12
    assert isinstance(reg.inplane_predictor[-1], torch.nn.Tanh) and float(cs.abs().max()) <= 1.0
    net.regressor.float()


def test_ist_live_sets_have_the_row_counts_they_are_named_after():
    B, k = 4, 3
    R = B * k * sr.P
    assert R == 3072 == 24 * 128 and sr.IST_LIVE_COUNTS == (0, 1, 127, 128, 129, 1280, 1281, R - 1, R)
    tar, src, order = sr.ist_points_case(7, B, k)
    assert sorted(order.tolist()) == list(range(R)) and order[0] >= R - sr.P
    assert tar.min() >= 0 and tar.max() <= 15 and src.min() >= 0 and src.max() <= 15
    prev = np.zeros(R, bool)
    for n in sr.IST_LIVE_COUNTS:
        tp, sp, live = sr.ist_live_set(tar, src, order, n)
        valid = ((tp != -1).all(-1) & (sp != -1).all(-1)).reshape(R)
        assert int(valid.sum()) == n == int(live.sum()) and (valid == live).all()
        assert (tp.reshape(R, 2)[live] == tar.reshape(R, 2)[live]).all() and (sp.reshape(R, 2)[live] == src.reshape(R, 2)[live]).all()
        assert (tp.reshape(R, 2)[~live] == -1).all() and (sp.reshape(R, 2)[~live] == -1).all()
        assert (live | ~prev).all()                                      # nested
        prev = live
        if n == 1:
            assert live[R - sr.P:].sum() == 1                            # the single live row sits in the last (b, j) block
    # half-specified rows: exactly one coordinate of a side is -1, and the oracle's validity rule calls them invalid
    tp, sp, live = sr.ist_live_set(tar, src, order, 1280)
    tp2, sp2, rows = sr.ist_half_specified(tp, sp, live, 9)
    t2, s2 = tp2.reshape(R, 2)[rows], sp2.reshape(R, 2)[rows]
    assert not live[rows].any() and len(set(rows.tolist())) == 64
    assert (((t2 == -1).sum(1) == 1) | ((s2 == -1).sum(1) == 1)).all() and ((t2 == -1).sum(1) <= 1).all() and ((s2 == -1).sum(1) <= 1).all()
    assert ((t2[:, 0] == -1) & (t2[:, 1] != -1)).any() and ((t2[:, 1] == -1) & (t2[:, 0] != -1)).any()
    assert ((s2[:, 0] == -1) & (s2[:, 1] != -1)).any() and ((s2[:, 1] == -1) & (s2[:, 0] != -1)).any()
    valid2 = ((tp2 != -1).all(-1) & (sp2 != -1).all(-1)).reshape(R)
    assert (valid2 == live).all()


def test_ist_gather_f64_and_the_oracle_agree_on_the_live_rows():
    """The float64 gather + regressor against the CPU oracle (f32 fmaf chains) on one live set: same rows, f32-class difference; a
    gather that exchanges x and y is noticed."""
    from oracle import cpu as oracle

    net, w = _ist(111)
    rs = np.random.RandomState(112)
    O, N, B, k = 2, 5, 4, 3
    bank = rs.standard_normal((O, N, 256, 256)).astype(np.float32)
    tarf = rs.standard_normal((B, 256, 256)).astype(np.float32)
    labels0 = rs.randint(0, O, B).astype(np.int32)
    ids = rs.randint(0, N, (B, k)).astype(np.int64)
    tar, src, order = sr.ist_points_case(113, B, k)
    tp, sp, live = sr.ist_live_set(tar, src, order, 129)
    osc, ocs = oracle.ist_inference(tarf, bank[labels0[:, None], ids], tp, sp, w)
    rows = np.nonzero(live)[0]
    assert ((osc.reshape(-1) == -1000) == ~live).all()
    sc, cs = sr.ist_regressor_f64(sr.ist_gather_f64(tarf, bank, labels0, ids, tp, sp, rows), w)
    mag = float(sc.abs().max())
    assert float((torch.from_numpy(osc.reshape(-1)[rows]).double() - sc).abs().max()) < 1e-5 * max(1.0, mag)
    assert float((torch.from_numpy(ocs.reshape(-1, 2)[rows]).double() - cs).abs().max()) < 1e-5
    swapped = sr.ist_gather_f64(tarf, bank, labels0, ids, tp, sp[..., ::-1], rows)
    sc2, _ = sr.ist_regressor_f64(swapped, w)
    assert float((sc2 - sc).abs().max()) > 1e-2 * max(1.0, mag)


# ---------------------------------------------------------------------------------------------------------------- split attention
def _attention_values(cls, B, H, seed, scale=8.0):
    hi, lo = sr.split_planes_host(sr.attention_case(cls, B, H, seed), scale)
    return sr.planes_value(hi, lo, scale)


def test_attention_ref_is_torchs_own_float64_attention():
    B, H = 2, 3
    vals = _attention_values("plain", B, H, 3)
    q, k, v = sr.attention_qkv(vals, B, H)
    want = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3)         # scale = 64^-0.5
    got = sr.attention_ref(vals, B, H)
    assert got.dtype == torch.float64 and got.shape == (B, sr.T_TOK, H, 64)
    assert float((got - want).abs().max()) < 1e-13
    # the layout: q | k | v blocks of 64 H channels per token row, head-major inside a block
    x = vals.reshape(B, sr.T_TOK, 3 * 64 * H)
    assert torch.equal(q[1, 2, 5], x[1, 5, 2 * 64:3 * 64]) and torch.equal(v[0, 1, 256], x[0, 256, 2 * 64 * H + 64:2 * 64 * H + 128])


@pytest.mark.parametrize("cls", sr.ATTN_CLASSES)
def test_attention_classes_hold_their_preconditions_and_the_reference_rejects_wrong_kernels(cls):
    """Per input class of tests/test_gpu_attention_split.py, at the ViT-L geometry, on the CPU: (1) the class's preconditions hold on
    the float64 logits, (2) the bound the kernel is held to is small against what a wrong kernel does: a kernel that drops key 256, one that
    scales by 1 / sqrt(63), one that takes every chunk of keys relative to its own maximum without rescaling -- each differs from the float64
    reference by more than 20 x the bound (where the class can see the bug at all: equal logits hide a wrong scale and a wrong maximum, the
    descending class gives key 256 no weight; those pairs are named below and shown to be blind, so nobody counts on them)."""
    B, H = 3, 16
    vals = _attention_values(cls, B, H, 5)
    pre = sr.attention_preconditions(cls, sr.attention_logits(vals, B, H))
    assert pre and all(ok for _, ok in pre.values()), pre
    ref = sr.attention_ref(vals, B, H)
    e32 = float((sr.attention_ref(vals, B, H, torch.float32).double() - ref).abs().max() / ref.abs().max())
    bound = sr.attention_bound(e32, 8.0)
    assert 1e-7 < e32 < 2e-4 and bound < 2e-4          # offset: ~7e-5 (the logit's own f32 rounding at |logit| ~ 300); every other < 1e-5
    if cls in ("uniform", "zero_q"):
        _, _, v = sr.attention_qkv(vals, B, H)
        mean = v.mean(dim=2, keepdim=True).expand(-1, -1, sr.T_TOK, -1).permute(0, 2, 1, 3)
        assert float((ref - mean).abs().max()) < 1e-14                                       # the reference IS the column mean of V
    blind = {"uniform": ("scale_63", "per_chunk_max"), "zero_q": ("scale_63", "per_chunk_max"),
             "descending": ("drop_key_256",)}.get(cls, ())      # descending: key 256 carries < 2^-15 of every row's weight
    for kind in ("drop_key_256", "scale_63", "per_chunk_max"):
        d = sr.attention_mutant(kind, vals, B, H) - ref
        err = float(d.abs().max() / ref.abs().max())
        err256 = float(d[:, 256].abs().max() / ref.abs().max())
        if kind in blind:
            assert err < 0.1 * bound, (kind, err)
            continue
        assert err > 20.0 * bound, (kind, err, bound)
        if kind == "drop_key_256":
            assert err256 > 20.0 * bound, (kind, err256, bound)      # query 256 has its own path to key 256: seen on that row alone too


def test_attention_preconditions_reject_another_class():
    """A generator that quietly stops producing its edge fails its precondition: each class's conditions, put to a case of another class."""
    B, H = 3, 16
    for cls, other in (("peaked", "plain"), ("plain", "peaked"), ("sink", "sink256"), ("sink256", "sink"), ("offset", "plain"),
                       ("uniform", "plain"), ("zero_q", "plain"), ("descending", "ascending"), ("ascending", "descending"),
                       ("descending", "peaked")):
        pre = sr.attention_preconditions(cls, sr.attention_logits(_attention_values(other, B, H, 5), B, H))
        assert not all(ok for _, ok in pre.values()), (cls, other, pre)


def test_attention_bound_is_the_stage_bound_for_plain_inputs():
    assert sr.attention_bound(9.0e-7, 8.0) == 2e-6 + 2.0 ** -21 and sr.attention_bound(9.0e-7, 0.5) == 4e-6 + 2.0 ** -21
    assert sr.attention_bound(7.2e-5, 8.0) == 1.44e-4 + 2.0 ** -21


# ---------------------------------------------------------------------------------------------------------------- f32 attention
# (tests/test_gpu_vit_f32_stages.py: attention_kernel reads f32 values, not planes -- the cases are attention_case's own f32 values)
def test_attention_bound_f32_has_no_plane_term():
    assert sr.attention_bound_f32(9.0e-7) == 2e-6 and sr.attention_bound_f32(7.2e-5) == 1.44e-4
    assert sr.attention_bound_f32(7.2e-5) == sr.attention_bound(7.2e-5, 8.0) - 2.0 ** -21


def test_attention_half_keys_are_frag_rows():
    """frag_row(r, lane) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (gp_common.h), restated: the two halves partition the 257 keys."""
    for half in (0, 1):
        rows = sorted(32 * t + (r & 3) + 8 * (r >> 2) + 4 * half for t in range(9) for r in range(16))
        assert sr.attention_half_keys(half).tolist() == [k for k in rows if k < sr.T_TOK]
    assert sorted(sr.attention_half_keys(0).tolist() + sr.attention_half_keys(1).tolist()) == list(range(sr.T_TOK))
    assert 256 in sr.attention_half_keys(0).tolist()


@pytest.mark.parametrize("B,H,Mpad", [(1, 6, 512), (3, 16, 1024), (5, 12, 1536)])
def test_attention_channel_major_layout_round_trip(B, H, Mpad):
    vals = sr.attention_case("plain", B, H, 5)
    C, M = 64 * H, B * sr.T_TOK
    qk, vt = sr.attention_cm_layout(vals, B, H, Mpad, float("nan"))
    assert qk.shape == (2 * C, Mpad) and vt.shape == (Mpad, C) and qk.dtype == vt.dtype == torch.float32
    # the layout, element by element: Q rows h * 64 + d, K rows C + h * 64 + d, column b * 257 + t; V token-major
    q, k, v = sr.attention_qkv(vals, B, H)
    b, h, t, d = B - 1, H - 2, 256, 37
    assert qk[h * 64 + d, b * 257 + t] == q[b, h, t, d] and qk[C + h * 64 + d, b * 257 + t] == k[b, h, t, d]
    assert vt[b * 257 + t, h * 64 + d] == v[b, h, t, d] and qk[5, 1] == q[0, 0, 1, 5]
    assert torch.isnan(qk[:, M:]).all() and torch.isnan(vt[M:]).all() and not torch.isnan(qk[:, :M]).any() and not torch.isnan(vt[:M]).any()
    back = sr.attention_cm_values(qk, vt, B, H)
    assert torch.equal(back, vals)
    assert torch.equal(sr.attention_ref(back.double(), B, H), sr.attention_ref(vals.double(), B, H))
    # ... and of the output
    ref = sr.attention_ref(vals.double(), B, H).float()
    out = sr.attention_cm_from_output(ref, Mpad, -7.0)
    assert out.shape == (C, Mpad) and out[h * 64 + d, b * 257 + t] == ref[b, t, h, d] and bool((out[:, M:] == -7.0).all())
    assert torch.equal(sr.attention_cm_output(out, B, H), ref)


@pytest.mark.parametrize("B,H", [(1, 6), (3, 16), (5, 12)])
@pytest.mark.parametrize("cls", sr.ATTN_CLASSES)
def test_attention_classes_hold_their_preconditions_on_the_f32_values(cls, B, H):
    """The geometries of tests/test_gpu_vit_f32_stages.py at its seed, ViT-S with one crop included."""
    pre = sr.attention_preconditions(cls, sr.attention_logits(sr.attention_case(cls, B, H, 5), B, H))
    assert pre and all(ok for _, ok in pre.values()), pre


# (mutant, class) pairs on which the class cannot see the bug -- every other pair must be separated:
#   scale_63, per_chunk_max, query_256_from_next_crop on uniform / zero_q: equal logits whatever the scale, the maximum or the query;
#   drop_key_256 on descending: key 256 carries < 2^-15 of every row's weight.
# So drop_key_256 bites on 8 classes (all but descending), scale_63 / per_chunk_max / query_256_from_next_crop on the 7 classes with
# unequal logits, half_denominator and channel_halves_swapped on all 9.
ATTN_F32_BLIND = {("scale_63", "uniform"), ("scale_63", "zero_q"), ("per_chunk_max", "uniform"), ("per_chunk_max", "zero_q"),
                  ("query_256_from_next_crop", "uniform"), ("query_256_from_next_crop", "zero_q"), ("drop_key_256", "descending")}


@pytest.mark.parametrize("cls", sr.ATTN_CLASSES)
def test_float64_attention_separates_every_mutant_from_the_f32_kernels_bound(cls):
    """ViT-L geometry (3 crops: a next crop exists), f32 values: each of the six wrong kernels is at least 10 x attention_bound_f32 away
    from the float64 reference on every class that can see it; the blind pairs are shown to be blind (< 0.1 x), so nobody counts on them."""
    B, H = 3, 16
    vals = sr.attention_case(cls, B, H, 5).double()
    ref = sr.attention_ref(vals, B, H)
    rmax = float(ref.abs().max())
    e32 = float((sr.attention_ref(vals, B, H, torch.float32).double() - ref).abs().max()) / rmax
    bound = sr.attention_bound_f32(e32)
    assert 1e-7 < e32 < 2e-4 and bound < 2e-4
    for kind in sr.ATTN_MUTANTS:
        d = sr.attention_mutant(kind, vals, B, H) - ref
        err, err256 = float(d.abs().max()) / rmax, float(d[:, 256].abs().max()) / rmax
        if (kind, cls) in ATTN_F32_BLIND:
            assert err < 0.1 * bound, (kind, cls, err, bound)
            continue
        assert err >= 10.0 * bound, (kind, cls, err, bound)
        if kind == "query_256_from_next_crop":
            assert err256 == err and float(d[:, :256].abs().max()) == 0.0      # that row alone
        if kind == "channel_halves_swapped":
            assert torch.equal(sr.attention_mutant(kind, vals, B, H)[..., :32], ref[..., 32:])


# ---------------------------------------------------------------------------------------------------------------- the split matcher
def _as_ours(name):
    case, ref, c = sr.match_case(name)
    return case, ref, c, sr.match_ref_as_ours(ref, case["B"], case["N"])


def test_match_tiles_f64_is_the_reference_formula_in_torch_float64():
    """The restatement against an independent one written with torch operators the way matching.py:233-278 does (masks multiply, threshold,
    torch.max first maximum, gather, cycle distance), on one tile with fractional masks, in both directions."""
    case, ref, _ = sr.match_case("blocks_a")
    b, n = 5, 6                                         # the two fractional rows
    q = (case["q_hi"][b].double() + case["q_lo"][b].double()) / 32.0
    t = (case["b_hi"][0, n].double() + case["b_lo"][0, n].double()) / 32.0
    qm, tm = torch.from_numpy(case["qm"][b]).double(), torch.from_numpy(case["tm"][0, n]).double()
    assert 0 < qm[qm > 0].min() < 1 and 0 < tm[tm > 0].min() < 1
    for direction in ("tar2src", "src2tar"):
        sim = (q @ t.t()) * tm[None, :] * qm[:, None]
        sim[sim < 0.3] = 0
        s_row, i_row = torch.max(sim, dim=1)
        s_col, i_col = torch.max(sim, dim=0)
        (sa, ia, sb, ib) = (s_row, i_row, s_col, i_col) if direction == "tar2src" else (s_col, i_col, s_row, i_row)
        p = torch.arange(256)
        back = ib[ia]
        dist = torch.sqrt(((back % 16 - p % 16) ** 2 + (back // 16 - p // 16) ** 2).double())
        m = (sa >= 0.3) & (dist <= 3.0) & (sb[ia] >= 0.3)
        mask = m.double() * qm * tm[ia] * (ib != 0).double() * (ia != 0).double()
        got = sr.match_tiles_f64(case["q_hi"], case["q_lo"], case["b_hi"], case["b_lo"], case["qm"], case["tm"], case["labels"], 0.3, 3.0,
                                 direction, tiles=[(b, n)])
        assert np.array_equal(got["idx"][0], ia.numpy())
        assert np.abs(got["score"][0] - sa.numpy()).max() < 1e-14
        assert np.abs(got["mask"][0].astype(np.float64) - mask.numpy()).max() < 1e-7 and (got["mask"][0] != 0).sum() == int((mask != 0).sum()) > 0
        assert abs(float(got["sim_avg"][0]) - float((sa * mask).sum() / 256.0)) < 1e-9


@pytest.mark.parametrize("name", list(sr.MATCH_CASES))
def test_match_cases_hold_their_preconditions_and_the_checker_accepts_the_reference(name):
    """Every case of tests/test_gpu_matcher_f64.py, on the CPU: what makes it the case it is named after holds, few decisions sit on a
    margin (so the cap on excused entries is a condition the reference alone meets by far), and match_tiles_check accepts
    match_tiles_f64's own records with nothing excused."""
    case, ref, c, ours = _as_ours(name)
    which, C, thr, pthr, direction, two_plane, O, anti, min_valid = sr.MATCH_CASES[name]
    assert (case["b_lo"] is not None) == two_plane and case["q_hi"].shape == (9, 256, C) and case["b_hi"].shape == (O, 9, 256, C)
    assert sr.planes_well_formed(case["q_hi"], case["q_lo"]) and (not two_plane or sr.planes_well_formed(case["b_hi"], case["b_lo"]))
    assert 2e-7 < c < 3e-6, c                                                  # a few f32 ulp of sum |q||b|
    valid = int((ref["mask"] != 0).sum())
    assert valid > min_valid, valid
    share = sr.match_near_margin_share(ref)
    assert share < sr.MATCH_EXCUSED_CAP / 10, share
    # live counts per row, the sentinel patches, the fractional rows
    qc, tc = (sr.MATCH_COUNTS_X, sr.MATCH_COUNTS_Y) if which == "a" else (sr.MATCH_COUNTS_Y, sr.MATCH_COUNTS_X)
    assert tuple((case["qm"] != 0).sum(-1)) == qc and all(tuple((case["tm"][o] != 0).sum(-1)) == tc for o in range(O))
    for m, counts in [(case["qm"], qc)] + [(case["tm"][o], tc) for o in range(O)]:
        for r, cnt in enumerate(counts):
            for p in (0, 255):
                if r % 2 == 1 and cnt >= 2:
                    assert m[r, p] != 0
                if r % 2 == 0 and cnt <= 254:
                    assert m[r, p] == 0
    fq, ft = sr.MATCH_FRAC_ROWS
    assert ((case["qm"][fq] > 0) & (case["qm"][fq] < 1)).sum() == qc[fq] and ((case["tm"][0, ft] > 0) & (case["tm"][0, ft] < 1)).sum() == tc[ft]
    assert set(np.unique(np.delete(case["qm"], fq, 0))) <= {0.0, 1.0}
    # the planted copies: bit-identical plane rows, live together, in different 32-row blocks of the compacted tile
    (t0, t1), (q0, q1) = sr.MATCH_DUP_TMPL, sr.MATCH_DUP_QUERY
    assert torch.equal(case["b_hi"][:, :, t0], case["b_hi"][:, :, t1]) and torch.equal(case["q_hi"][:, q0], case["q_hi"][:, q1])
    assert torch.equal(case["q_lo"][:, q0], case["q_lo"][:, q1]) and (not two_plane or torch.equal(case["b_lo"][:, :, t0], case["b_lo"][:, :, t1]))
    def blocks_apart(m, a, b):
        live = m != 0
        rank = np.cumsum(live, -1) - 1
        return (live[:, a] & live[:, b] & (rank[:, a] // 32 != rank[:, b] // 32)).sum()
    assert blocks_apart(case["tm"][0], t0, t1) >= 4 and blocks_apart(case["qm"], q0, q1) >= 4
    tie_rows = int(((ref["row_margin"] == 0) & (ref["row_v"] > 0)).sum())
    tie_cols = int(((ref["col_margin"] == 0) & (ref["col_v"] > 0)).sum())
    assert (tie_rows >= 5 or anti) and tie_cols >= 5, (tie_rows, tie_cols)    # exact ties between positive values exist on both sides (anti: the copies seldom lead a row)
    if anti:      # live rows whose maximum is a masked-out patch's exact zero, and live negative maxima where nothing is masked out
        live_rows = ref["qm"] != 0
        assert ((ref["score"] == 0) & (ref["idx"] != 0) & live_rows).sum() > 100 and (ref["score"] < 0).sum() > 100
    if thr == 0.0:
        assert (ref["U"] < 0).sum() > 10000                                   # negative similarities exist and are zeroed
    rep = sr.match_tiles_check(ours, ref, c)
    assert rep["failed"] == 0 and rep["excused"] == 0 and rep["checked"] == 81 * 257, rep


def test_match_block_cases_cover_all_81_live_block_layouts():
    seen = set()
    for name in ("blocks_a", "blocks_b"):
        case, _, _ = sr.match_case(name)
        lay = sr.match_case_layouts(case["qm"], case["tm"], case["labels"])
        assert len(lay) == 81                                                 # each of the two alone, the other with the sides exchanged
        seen |= lay
    assert seen == {(r, c) for r in range(9) for c in range(9)}
    case, _, _ = sr.match_case("three_objects")
    assert tuple(case["labels"]) == sr.MATCH_O3_LABELS and not torch.equal(case["b_hi"][0], case["b_hi"][1])
    assert len(sr.match_case_layouts(case["qm"], case["tm"], case["labels"])) == 81


@pytest.mark.parametrize("kind", sr.MATCH_MUTANTS)
def test_match_checker_rejects_subtly_wrong_matchers(kind):
    """Seven wrong results derived from the float64 one, each a bug the kernel could have: the checker reports failures for every one and
    excuses none of them away (the failures are not near any margin)."""
    case, ref, c = sr.match_case("blocks_a")
    rep = sr.match_tiles_check(sr.match_mutant(kind, case, ref), ref, c)
    assert rep["failed"] > 0 and rep["first"], (kind, rep)
    floor = {"tie_higher": 10, "zero_row_first_live": 1000, "colmax_drops_a_row_group": 100, "last_band_transposed": 100,
             "wrong_direction": 1000, "avg_by_count": 30, "score_offset": 1000}[kind]
    assert rep["failed"] >= floor, (kind, rep)


def test_match_checker_rejects_column_ties_and_wrong_direction_in_src2tar():
    """The column side of the tie rule shows in the index output of src2tar: query patch 250 (the copy) returned where 11 must be."""
    case, ref, c, ours = _as_ours("src2tar")
    q0, q1 = sr.MATCH_DUP_QUERY
    tied = (ours["idx"] == q0) & (ours["score"] != 0) & ((case["qm"][:, q0] == case["qm"][:, q1]) & (case["qm"][:, q1] != 0))[:, None, None]
    assert tied.sum() >= 5
    ours["idx"][tied] = q1
    rep = sr.match_tiles_check(ours, ref, c)
    assert rep["failed"] >= tied.sum() and "exact tie" in rep["first"]
    rep = sr.match_tiles_check(sr.match_mutant("wrong_direction", case, ref, direction="src2tar"), ref, c)
    assert rep["failed"] > 1000


def test_match_checker_excuses_only_what_sits_on_a_margin():
    """A flip to the runner-up passes as EXCUSED when the float64 margin is below eps = 2 c mag and fails when it is not; a score
    zeroed against the threshold likewise."""
    case, ref, c, ours = _as_ours("blocks_a")
    k = int(np.argmax((ref["mask"] != 0).sum(-1)))
    b, n = ref["tiles"][k]
    p = int(np.flatnonzero(ref["mask"][k] != 0)[0])
    U = ref["U"][k]
    second = int(np.argsort(U[p])[-2])
    margin = U[p, ref["idx"][k][p]] - U[p, second]
    assert margin > 1e-3
    ours["idx"][b, n, p], ours["score"][b, n, p] = second, np.float32(U[p, second])
    bad = sr.match_tiles_check(ours, ref, c)
    assert bad["failed"] >= 1 and bad["excused"] == 0 and f"det {b} template {n} patch {p}" in bad["first"]
    wide = sr.match_tiles_check(ours, ref, margin)             # the same flip under a coefficient as large as the margin: on the margin
    assert wide["excused"] >= 1 and "index" not in (wide["first"] or "")
    ours = sr.match_ref_as_ours(ref, 9, 9)
    ours["idx"][b, n, p], ours["score"][b, n, p] = 0, 0.0      # zeroed although the maximum is far above the threshold
    assert sr.match_tiles_check(ours, ref, c)["failed"] >= 1


# ---------------------------------------------------------------------------------------------------------------- IST convolutions at the ends of the range
def _range_ref(name):
    case = sr.conv_range_named(name)
    wide = sr.CONV_RANGE_CASES[name][2]
    x, w, r = sr.conv_case_values(case, wide)
    return case, wide, sr.conv_range_reference(x, w, case["alpha"], case["beta"], r, case["stride"], case["pad"])


def test_wide_host_split_reconstructs_to_22_bits():
    x = torch.from_numpy(sr.split_values_case(4096, 3)) * 8.0          # up to 64000
    hi, lo = sr.split_wide_host(x)
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all())
    err = (sr.wide_value(hi, lo) - x.double()).abs()
    assert bool((err <= sr.WIDE_FLOOR[0] * x.double().abs() + sr.WIDE_FLOOR[1]).all())
    assert bool((sr.wide_value(hi, lo).float().double() == sr.wide_value(hi, lo)).all())       # the values fit f32: torch's f32 evaluation reads them exactly


@pytest.mark.parametrize("name", list(sr.CONV_RANGE_CASES))
def test_conv_range_cases_hold_their_preconditions(name):
    """Values from 1e-4 to the thousands, the planted specials where the builder says, a float64 peak of |format y| between 0.5 and 0.95 of 65504,
    outputs 1000 times smaller than the largest present, and torch's own f32 evaluation inside the bound with err / bound <= 0.5 by construction."""
    case, wide, ref = _range_ref(name)
    X = np.abs(case["X"])
    assert X[X > 0].min() < 1e-3 and (2000.0 if not wide else 15000.0) < X.max() < case["limit"] and 0.3 < case["factor"] < 3.0
    special = sr.split_values_case(40, 0)[1:23]                               # the specials do not depend on the seed
    assert np.array_equal(case["X"][case["planted_x"]][:case["n_special"]], special[:case["n_special"]])
    assert 1024.0 in case["R"][case["planted_r"]] and 1.0 + 2.0 ** -11 in case["R"][case["planted_r"]]
    peak = float(ref["y"].abs().max()) * (1.0 if wide else 8.0) / sr.F16_MAX
    y = ref["y"]
    small = int(((y > 0) & (y < 1e-3 * y.max())).sum())
    worst32, _ = sr.conv_bound_worst(ref["y32"], ref, None)
    print(f"{name}: factor {case['factor']:.3f}, peak {peak:.3f} of 65504, c {ref['c']:.3e}, outputs below 1e-3 max: {small}, torch f32 err / bound {worst32:.3f}")
    assert 0.5 <= peak <= 0.95 and small >= 10
    assert worst32 <= 0.5 + 1e-12
    floor = sr.WIDE_FLOOR if wide else sr.PLANES_FLOOR
    assert sr.conv_bound_worst(ref["y"], ref, floor)[0] == 0.0
    # the plane format's own rounding of the float64 result sits inside its floor term
    yh = ref["y"].float()
    back = sr.wide_value(*sr.split_wide_host(yh)) if wide else sr.planes_value(*sr.split_planes_host(yh, 8.0), 8.0)
    assert bool(((back - yh.double()).abs() <= floor[0] * yh.double().abs() + floor[1]).all())


@pytest.mark.parametrize("kind", sr.CONV_MUTANTS)
@pytest.mark.parametrize("name", list(sr.CONV_RANGE_CASES))
def test_conv_bound_rejects_subtly_wrong_convolutions(name, kind):
    """Activation lo planes dropped / the residual added as its hi plane only / outputs below 2^-10 max |y| flushed to zero: each derived from
    the float64 result, each outside the bound (plane floor included) on every case."""
    case, wide, ref = _range_ref(name)
    worst, at = sr.conv_bound_worst(sr.conv_mutant(kind, case, wide), ref, sr.WIDE_FLOOR if wide else sr.PLANES_FLOOR)
    print(f"{name} / {kind}: worst err / bound {worst:.3g} at {at}")
    assert worst > 2.0


def test_conv_bound_counts_a_non_finite_output_as_a_miss():
    case, wide, ref = _range_ref("gather_ni3_1x1")
    bad = ref["y"].clone()
    bad[0, 5, 3, 3] = float("inf")
    assert sr.conv_bound_worst(bad, ref, sr.PLANES_FLOOR)[0] == float("inf")
    assert sr.conv_bound_worst(bad, ref, sr.PLANES_FLOOR, where=torch.isfinite(bad))[0] == 0.0


@pytest.mark.parametrize("route", list(sr.CONV_GUARD_ROUTES))
def test_conv_guard_cases_sit_where_they_say(route):
    """Launch preconditions of gp_conv2d_planes; the zero-weight channel's float64 value is v exactly at every pixel and everything else small;
    the residual cases' float64 output is beyond 8190 x 1.01 (over) / everything below 8190 x 0.99 (clean), every OPERAND a legal plane value."""
    cin, cout, k, stride, pad, hw, B = sr.CONV_GUARD_ROUTES[route]
    assert cin % 32 == 0 and cout % 64 == 0 and (B * sr.conv_out_size(hw, k, stride, pad) ** 2) % 256 == 0
    for v in (8188.0, 8188.5, -8188.5):
        case = sr.conv_guard_zero_channel_case(route, v)
        x, w, _ = sr.conv_case_values(case)
        y = sr.conv_range_reference(x, w, case["alpha"], case["beta"], None, case["stride"], case["pad"], relu=False)["y"]
        assert bool((y[:, case["co"]] == v).all())
        rest = torch.cat([y[:, :case["co"]], y[:, case["co"] + 1:]], dim=1)
        assert float(rest.abs().max()) < 20.0
    for where in ("first", "last"):
        for over in (False, True):
            case = sr.conv_guard_residual_case(route, where, over)
            assert (case["pix"], case["co"]) == ((0, 0) if where == "first" else (case["npix"] - 1, cout - 1))
            assert np.abs(case["R"]).max() * 8.0 < sr.F16_MAX and np.abs(case["X"]).max() < 10.0
            x, w, r = sr.conv_case_values(case)
            y = sr.conv_range_reference(x, w, case["alpha"], case["beta"], r, case["stride"], case["pad"])["y"]
            y = y.permute(0, 2, 3, 1).reshape(case["npix"], cout)
            at = float(y[case["pix"], case["co"]])
            y[case["pix"], case["co"]] = 0.0
            assert float(y.max()) < 0.99 * 8190.0 and (at > 1.01 * 8190.0 if over else at < 0.99 * 8190.0)


def test_resize_guard_images_peak_where_they_say():
    for over, peak in ((False, 8100.0), (True, 8300.0)):
        assert float(sr.resize_f64(sr.resize_guard_image(over), 32).abs().max()) == peak
    assert 8300.0 >= 8190.0 * 1.01 and 8100.0 <= 8190.0 * 0.99


def test_resnet_layer_maxima_is_the_torch_forward():
    """The traced forward returns ist_torch.resnet_forward's features, and `written` holds what the split path stores: the positive part after
    bn1, the shortcut's BatchNorm output, block outputs -- on a tiny ResNet."""
    from gigapose_amd.ist_net import ResNet
    from gigapose_testing import synthetic as syn
    from oracle import ist_torch

    net = syn.fill_state_dict(ResNet(dict(n_heads=0, input_dim=3, input_size=32, initial_dim=8, block_dims=[8, 16, 16, 32], descriptor_size=8)), 4).eval().double()
    x = torch.randn(2, 3, 20, 28, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    rec, written, feats = sr.resnet_layer_maxima(net, x)
    with torch.no_grad():
        assert torch.equal(feats, ist_torch.resnet_forward(net, x))
    assert "relu(bn1)" in written and "relu(layer3.1.bn1)" in written and "layer2.0.downsample.1" in written and "layer4.1.out" in written
    assert "conv1" in rec and "conv1" not in written and "layer1.0.bn2" in rec and "layer1.0.bn2" not in written
    assert all(v <= rec[n[5:-1]] for n, v in written.items() if n.startswith("relu("))
    assert len(written) == 1 + 1 + 8 + 3 + 8
