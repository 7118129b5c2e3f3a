"""GPU: the f32 ViT kernels that run whenever gp_vit_forward is off the plane path (gp_vit.hip: attention_kernel / attention_body,
layernorm_wide_kernel, im2col_kernel + embed_kernel, features_kernel), each on its own against float64 or a bit-exact restatement.

These kernels carry ViT-S/14 (width 384 never takes the plane path), ViT-L below 8 crops, the automatic fall-back after a range trip
and the whole `chain` mode; the feature epilogue and the embedding run on every forward.  Until now only whole-ViT comparisons on
random-init weights (a nearly uniform softmax) reached them.  The stage entries gp_vit_attention_f32 / gp_vit_layernorm_f32 /
gp_vit_features live in the probe library (include/gigapose_hip_probe.h: the product header is at its bar of 45 entry points) and go
through the launchers the forward uses; test_one_block_composed_from_the_stage_entries_equals_the_product_forward ties the product
binary's kernels to them bit for bit.

  * attention: the nine input classes of gigapose_testing/stage_refs.py (attention_case; what each drives to an edge is said there) at
    ViT-S x 1 crop (54 wave-blocks: less than one XCD chunk, 255 pad columns), ViT-L x 3 and ViT-B x 5 (540 blocks: the `q < 0` tail of
    xcd_chunked_tile runs).  Bound stage_refs.attention_bound_f32 = max(2 e32, 2e-6) on max |err| / max |ref|, e32 = torch's own f32
    evaluation on the CPU on the same values.  tests/test_stage_refs.py shows without a GPU that float64 separates six wrong kernels
    (among them: the denominator of one lane half, o0 / o1 exchanged, query 256 from the next crop) from that bound by 10 x.
  * LayerNorm: stage_refs.layernorm_case at per = C / 16 = 8, 24, 64, 80 channels per slice; per token class at most
    max(LN_MARGIN x ATen f32, LN_MODEL_MARGIN x numpy f32 model of 16 contiguous slices) + 2^-24 (one f32 rounding of y; margins as
    in test_gpu_layernorm_planes.py); and, with no tolerance, equal to layernorm_planes_kernel's planes where the product dispatches to it.
  * features: bit-equal to oracle.l2norm_cp (the same sequential fma chain); NaN in every column the kernel has no business reading.
  * embedding: bit-equal to the oracle's chain GEMM over K = 592 + one f32 add, on the product library.
Measured figures: profiles/stage_tests_f32_vit.txt.  Arithmetic restated: HF modeling_dinov2.py:97-112, :207-229, :342-380; ae_net.py:64-69."""
import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from gigapose_testing import synthetic as syn
from oracle import cpu as oracle
from test_gpu_layernorm_planes import LN_MARGIN, LN_MODEL_MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
NAN = float("nan")
SENTINEL = 1234.5
F = torch.nn.functional


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def bits(t):
    return t.contiguous().view(torch.int32)


def round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------- 3.1 attention
def attention_f32(qk, vt, B, H, Mpad):
    """qk [2 * 64 H][Mpad], vt [Mpad][64 H] on the CPU -> out [64 H][Mpad] on the CPU, pre-filled with the sentinel."""
    dqk, dvt = qk.to(DEV), vt.to(DEV)
    out = torch.full((64 * H, Mpad), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.call("gp_vit_attention_f32", _lib.ptr(dqk), _lib.ptr(dvt), _lib.ptr(out), _lib.i(B), _lib.i(H), _lib.i(64 * H), _lib.i(Mpad),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.probes
@pytest.mark.parametrize("cls", sr.ATTN_CLASSES)
@pytest.mark.parametrize("B,H", [(1, 6), (3, 16), (5, 12)])
def test_attention_f32_vs_float64_on_adversarial_inputs(B, H, cls):
    M = B * sr.T_TOK
    Mpad = round_up(M, 256)
    assert Mpad == {1: 512, 3: 1024, 5: 1536}[B]
    vals32 = sr.attention_case(cls, B, H, seed=5)
    vals = vals32.double()                                          # what the kernel is given, in float64
    pre = sr.attention_preconditions(cls, sr.attention_logits(vals, B, H))
    assert pre and all(ok for _, ok in pre.values()), f"class {cls} is no longer what it is named after: {pre}"
    ref = sr.attention_ref(vals, B, H)
    rmax = float(ref.abs().max())
    e32 = float((sr.attention_ref(vals, B, H, torch.float32).double() - ref).abs().max()) / rmax
    bound = sr.attention_bound_f32(e32)
    if cls in ("uniform", "zero_q"):
        mean = sr.attention_qkv(vals, B, H)[2].mean(dim=2, keepdim=True).expand(-1, -1, sr.T_TOK, -1).permute(0, 2, 1, 3)
        assert float((ref - mean).abs().max()) < 1e-14

    qk, vt = sr.attention_cm_layout(vals32, B, H, Mpad, NAN)         # pad columns / rows: NaN, the kernel has no business reading them
    out = attention_f32(qk, vt, B, H, Mpad)
    _lib.check_status()
    got = sr.attention_cm_output(out, B, H).double()
    finite = bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max()) / rmax
    err256 = float((got[:, 256] - ref[:, 256]).abs().max()) / rmax
    print(f"attention f32 {cls:10s} B={B} H={H}: kernel {err:.3e}  f32 CPU reference {e32:.3e}  ratio {err / e32:.2f}  bound {bound:.3e}  "
          f"kernel / bound {err / bound:.3f}  query 256 alone {err256:.3e}")
    assert finite, "a non-finite output on a token column: a pad column / row was read"
    assert err <= bound, f"{err:.3e} > {bound:.3e} ({err / e32:.2f} x the f32 reference's error)"
    assert err256 <= bound, f"query 256: {err256:.3e} > {bound:.3e}"
    # columns >= B * 257 are nobody's: still the sentinel
    assert bool((out[:, M:] == SENTINEL).all()), "pad columns of the output were written"
    # a second launch is bit-equal to the first
    assert torch.equal(bits(attention_f32(qk, vt, B, H, Mpad)), bits(out)), "attention_kernel is not deterministic"
    # position independence: crops and heads permuted (independently) on the way in -> the same permutation of the first output, bit for bit
    pb = torch.roll(torch.arange(B), 1)
    ph = torch.from_numpy(np.random.RandomState(17 + H).permutation(H))
    assert not torch.equal(ph, torch.arange(H))
    pv = vals32.reshape(B, sr.T_TOK, 3, H, 64)[pb][:, :, :, ph].reshape(M, 3 * 64 * H).contiguous()
    qk2, vt2 = sr.attention_cm_layout(pv, B, H, Mpad, NAN)
    got2 = sr.attention_cm_output(attention_f32(qk2, vt2, B, H, Mpad), B, H)
    _lib.check_status()
    want2 = sr.attention_cm_output(out, B, H)[pb][:, :, ph]
    assert torch.equal(bits(got2), bits(want2)), "the output of a (crop, head) depends on where it sits in the batch"


@pytest.mark.probes
def test_attention_f32_argument_errors():
    B, H, Mpad = 1, 2, 512
    qk = torch.zeros(2 * 64 * H, Mpad, device=DEV)
    vt = torch.zeros(Mpad, 64 * H, device=DEV)
    out = torch.zeros(64 * H, Mpad, device=DEV)

    def call(**kw):
        a = dict(qk=qk, vt=vt, out=out, B=B, H=H, dim=64 * H, Mpad=Mpad)
        a.update(kw)
        _lib.call("gp_vit_attention_f32", _lib.ptr(a["qk"]), _lib.ptr(a["vt"]), _lib.ptr(a["out"]), _lib.i(a["B"]), _lib.i(a["H"]), _lib.i(a["dim"]),
                  _lib.i(a["Mpad"]), _lib.stream_ptr())

    call()
    for bad in (dict(qk=None), dict(vt=None), dict(out=None), dict(dim=64 * H + 64), dict(Mpad=256), dict(Mpad=384), dict(B=2), dict(B=0), dict(H=0, dim=0)):
        with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_vit_attention_f32"):
            call(**bad)
    torch.cuda.synchronize()
    _lib.check_status()


# ---------------------------------------------------------------------------------------------------------------- 3.2 LayerNorm
def layernorm_f32(x_tm, gamma, beta):
    """x_tm [Mpad][C] f32 on the CPU (token-major) -> y [Mpad][C] f32 on the CPU; the kernel reads and writes [C][Mpad]."""
    Mpad, C = x_tm.shape
    X = x_tm.to(DEV).t().contiguous()
    Y = torch.full((C, Mpad), SENTINEL, dtype=torch.float32, device=DEV)
    g, b = gamma.to(DEV), beta.to(DEV)
    _lib.call("gp_vit_layernorm_f32", _lib.ptr(X), _lib.ptr(Y), _lib.ptr(g), _lib.ptr(b), _lib.i(C), _lib.i(Mpad), _lib.f(EPS), _lib.stream_ptr())
    torch.cuda.synchronize()
    return Y.t().contiguous().cpu()


@pytest.mark.probes
@pytest.mark.parametrize("Mpad", [512, 2304])
@pytest.mark.parametrize("C", [128, 384, 1024, 1280])
def test_layernorm_f32_vs_float64(C, Mpad):
    """layernorm_wide_kernel: 16 contiguous slices of per = C / 16 channels (8: one unroll group, 24: a ragged one, 64: ViT-L, 80)."""
    seed = 100 + C + Mpad
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, seed)
    y = layernorm_f32(x, gamma, beta)
    _lib.check_status()
    y64, xhat = sr.layernorm_f64(x, gamma, beta, EPS)
    ref = sr.per_class_max(sr.layernorm_error(F.layer_norm(x, (C,), gamma, beta, EPS), y64, xhat, gamma, beta), cls)
    model_y = torch.from_numpy(sr.layernorm_partial_sums_f32(x.numpy(), gamma.numpy(), beta.numpy(), EPS, 16, contiguous=True))
    model = sr.per_class_max(sr.layernorm_error(model_y, y64, xhat, gamma, beta), cls)
    got = sr.per_class_max(sr.layernorm_error(y, y64, xhat, gamma, beta), cls)
    bound = {k: max(LN_MARGIN * ref[k], LN_MODEL_MARGIN * model[k]) + 2.0 ** -24 for k in ref}     # 2^-24: the one f32 rounding of y
    assert set(got) == set(sr.LN_CLASSES)
    for k in got:
        print(f"LN f32 C={C} Mpad={Mpad} class {k:8s}: kernel {got[k]:.3e}  f32 CPU reference {ref[k]:.3e}  ratio "
              f"{got[k] / ref[k] if ref[k] else float('nan'):.2f}  bound {bound[k]:.3e}  kernel / bound {got[k] / bound[k]:.3f}  "
              f"(numpy f32 model of 16 contiguous slices {model[k]:.3e}; bit-equal to it: {bool(torch.equal(bits(y[cls == sr.LN_CLASSES.index(k)]), bits(model_y[cls == sr.LN_CLASSES.index(k)])))})")
    assert bool(torch.isfinite(y).all())
    for k in got:
        assert got[k] <= bound[k], (k, got[k], ref[k], model[k], bound[k])
    # constant and pad tokens: x - mean is exactly 0 in any summation order -> y == beta, bit for bit
    flat = (cls == 3) | (cls == 4)
    assert int(flat.sum()) >= 10
    assert torch.equal(bits(y[flat]), bits(beta.expand(int(flat.sum()), C))), "constant / pad tokens: y != beta"
    # position independence: the arithmetic of a token does not depend on its lane, block or neighbours
    perm = torch.from_numpy(np.random.RandomState(seed + 1).permutation(Mpad))
    assert torch.equal(bits(layernorm_f32(x[perm], gamma, beta)), bits(y[perm])), "a token's LayerNorm depends on its column"
    _lib.check_status()


@pytest.mark.parametrize("Mpad", [512, 2304])
@pytest.mark.parametrize("C", [384, 1280])
def test_layernorm_f32_equals_the_plane_kernel_bit_for_bit(C, Mpad):
    """gp_vit.hip promises that layernorm_planes_kernel has "the same arithmetic" as layernorm_wide_kernel, "so y is bit-identical".  At
    these widths the PRODUCT library's gp_layernorm_planes dispatches to that kernel (launch_layernorm_planes: neither 1024 nor 768): its
    planes must be the host split of the f32 entry's y, bit for bit -- no tolerance."""
    x, cls, gamma, beta = sr.layernorm_case(C, Mpad, 100 + C + Mpad)
    X = x.to(DEV).t().contiguous()
    g, b = gamma.to(DEV), beta.to(DEV)
    hi = torch.zeros(Mpad, C, dtype=torch.float16, device=DEV)
    lo = torch.zeros_like(hi)
    _lib.call("gp_layernorm_planes", _lib.ptr(X), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(g), _lib.ptr(b), _lib.i(C), _lib.i(Mpad), _lib.f(EPS),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    with _lib.probe_library():
        y = layernorm_f32(x, gamma, beta)
    _lib.check_status()
    whi, wlo = sr.split_planes_host(y, 8.0)
    nh, nl = int((hi.cpu().view(torch.int16) != whi.view(torch.int16)).sum()), int((lo.cpu().view(torch.int16) != wlo.view(torch.int16)).sum())
    print(f"LN f32 vs planes kernel C={C} Mpad={Mpad}: {nh} hi and {nl} lo plane elements of {Mpad * C} differ from split(8 y_f32)")
    assert nh == 0 and nl == 0


@pytest.mark.probes
def test_layernorm_f32_argument_errors():
    x = torch.zeros(128, 128, device=DEV)
    y = torch.zeros_like(x)
    g = torch.ones(128, device=DEV)

    def call(**kw):
        a = dict(X=x, Y=y, ga=g, be=g, C=128, Mpad=128)
        a.update(kw)
        _lib.call("gp_vit_layernorm_f32", _lib.ptr(a["X"]), _lib.ptr(a["Y"]), _lib.ptr(a["ga"]), _lib.ptr(a["be"]), _lib.i(a["C"]), _lib.i(a["Mpad"]),
                  _lib.f(EPS), _lib.stream_ptr())

    call()
    for bad in (dict(C=120), dict(C=0), dict(Mpad=96), dict(Mpad=0), dict(X=None), dict(Y=None), dict(ga=None), dict(be=None)):
        with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_vit_layernorm_f32"):
            call(**bad)
    torch.cuda.synchronize()
    _lib.check_status()


# ---------------------------------------------------------------------------------------------------------------- 3.3 features
def features(X, B, C, Mpad, normalize):
    out = torch.full((B, C, 256), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.call("gp_vit_features", _lib.ptr(X), _lib.ptr(out), _lib.i(B), _lib.i(C), _lib.i(Mpad), _lib.i(normalize), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


def zero_token(b):
    return 1 + (17 * b + 5) % 256


def features_case(B, C, seed):
    """X [C][Mpad] f32: patch tokens N(0, 1) x a per-token scale 10^U(-3, 3); one patch token per crop all zeros (the 1e-12 clamp); the
    class-token column of every crop and every pad column NaN.  -> X, and the patch tokens as (B, C, 256)."""
    rs = np.random.RandomState(seed)
    Mpad = round_up(B * 257, 256)
    tok = (rs.standard_normal((B, 257, C)) * 10.0 ** rs.uniform(-3.0, 3.0, (B, 257, 1))).astype(np.float32)
    for b in range(B):
        tok[b, zero_token(b)] = 0.0
    tok[:, 0] = np.nan
    X = np.full((C, Mpad), np.nan, np.float32)
    X[:, :B * 257] = tok.reshape(B * 257, C).T
    return torch.from_numpy(X), np.ascontiguousarray(tok[:, 1:].transpose(0, 2, 1)), Mpad


@pytest.mark.probes
@pytest.mark.parametrize("B,C", [(1, 384), (16, 384), (64, 1024)])
def test_features_bit_exact_and_guarded(B, C):
    """The three grid shapes of launch_features: 32, 16 and 4 channel chunks per crop."""
    Xc, patches, Mpad = features_case(B, C, 300 + B + C)
    X = Xc.to(DEV)
    # normalize = 1: the oracle's sequential fma chain, bit for bit; NaN columns never read (output finite, status clean)
    got = features(X, B, C, Mpad, 1).cpu().numpy()
    _lib.check_status()
    want = oracle.l2norm_cp(patches)
    assert np.isfinite(got).all(), "the class-token column or a pad column was read"
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    for b in range(B):
        assert not got[b, :, zero_token(b) - 1].any(), "an all-zero token must give zeros (1e-12 clamp)"
    # normalize = 0: an exact copy
    raw = features(X, B, C, Mpad, 0).cpu().numpy()
    _lib.check_status()
    np.testing.assert_array_equal(raw.view(np.uint32), patches.view(np.uint32))
    # the guard: one bad value in one patch token raises the range bit with normalize = 1 -- and only there
    spot = (C - 1, (B - 1) * 257 + 256)                  # the last channel of the last token of the last crop
    for name, v in (("NaN", NAN), ("+inf", float("inf")), ("sum x^2 > 3e38", 1.8e19)):
        Xb = X.clone()
        Xb[spot] = v
        if name.startswith("sum"):
            assert np.isfinite(np.float32(v) * np.float32(v)) and float(np.float32(v) * np.float32(v)) > 3.0e38     # finite, above the guard's limit
        features(Xb, B, C, Mpad, 1)
        with pytest.raises(_lib.GigaPoseHipError, match="range of the f16 planes"):
            _lib.check_status()
        assert _lib.take_status() == 0
        rawb = features(Xb, B, C, Mpad, 0)
        _lib.check_status()                              # normalize = 0 copies the values as they are: no bit
        assert torch.equal(bits(rawb[B - 1, C - 1, 255:].cpu()), bits(torch.tensor([v], dtype=torch.float32)))


@pytest.mark.probes
def test_features_argument_errors():
    X = torch.zeros(128, 256 * 3, device=DEV)
    out = torch.zeros(2, 128, 256, device=DEV)

    def call(**kw):
        a = dict(X=X, out=out, B=2, C=128, Mpad=768)
        a.update(kw)
        _lib.call("gp_vit_features", _lib.ptr(a["X"]), _lib.ptr(a["out"]), _lib.i(a["B"]), _lib.i(a["C"]), _lib.i(a["Mpad"]), _lib.i(1), _lib.stream_ptr())

    call()
    for bad in (dict(X=None), dict(out=None), dict(B=0), dict(C=0), dict(Mpad=512), dict(Mpad=0)):
        with pytest.raises(_lib.GigaPoseHipError, match=r"rc=-1.*gp_vit_features"):
            call(**bad)
    torch.cuda.synchronize()
    _lib.check_status()


# ---------------------------------------------------------------------------------------------------------------- 3.4 embedding
def make_vit(dim, depth, seed):
    from gigapose_amd.vit import Dinov2ViT

    vit = syn.fill_state_dict(Dinov2ViT(dim, depth, dim // 64), seed).eval().to(DEV)
    return vit.set_numerics("chain")


def forward_with_nan_workspace(vit, x, stop):
    """gp_vit_forward through Dinov2ViT.patch_features (normalize = 0) on a workspace pre-filled with NaN -> out (B, dim, 256) and
    the workspace's x_prenorm^T [dim][Mpad] (include/gigapose_hip.h), both on the CPU."""
    B = x.shape[0]
    ws, _ = vit._workspace(B, x.device)
    ws.fill_(NAN)
    out = vit.patch_features(x, normalize=False, stop_after_layers=stop)
    torch.cuda.synchronize()
    _lib.check_status()
    Mpad = round_up(B * 257, 256)
    assert vit._ws is ws
    return out.reshape(B, vit.dim, 256).cpu(), ws[:vit.dim * Mpad].view(vit.dim, Mpad).clone()


def im2col_host(x):
    """(B, 3, 224, 224) -> [592][B * 256]: row k = ci * 196 + dy * 14 + dx, column b * 256 + py * 16 + px; rows 588..591 zero."""
    B = x.shape[0]
    col = np.zeros((592, B * 256), np.float32)
    col[:588] = x.reshape(B, 3, 16, 14, 16, 14).transpose(1, 3, 5, 0, 2, 4).reshape(588, B * 256)
    return col


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dim", [128, 384])
def test_embedding_bit_exact_vs_the_chain_gemm(dim, B):
    vit = make_vit(dim, 1, 31)
    x = torch.from_numpy(np.random.RandomState(32 + B).standard_normal((B, 3, 224, 224)).astype(np.float32))
    out, X = forward_with_nan_workspace(vit, x.to(DEV), 0)
    X = X.cpu().numpy()
    M, Mpad = B * 257, round_up(B * 257, 256)
    patch_wt, patch_b, cls_pos, pos_t = (t.cpu().numpy() for t in vit._packed[1][:4])
    assert patch_wt.shape == (592, dim) and not patch_wt[588:].any()
    pe = oracle.gemm_kmajor(patch_wt, im2col_host(x.numpy()), 1, patch_b)                     # [dim][B * 256], the fmaf chain over k = 0 .. 591 + bias
    want = (pe.reshape(dim, B, 256) + pos_t[:, None, :]).astype(np.float32)                    # one f32 add
    tok = X[:, :M].reshape(dim, B, 257)
    np.testing.assert_array_equal(tok[:, :, 1:].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(tok[:, :, 0].view(np.uint32), np.ascontiguousarray(np.broadcast_to(cls_pos[:, None], (dim, B))).view(np.uint32))
    assert Mpad > M and not X[:, M:].view(np.uint32).any(), "pad columns of the residual stream are not exactly +0.0"
    np.testing.assert_array_equal(out.numpy().view(np.uint32), np.ascontiguousarray(tok[:, :, 1:].transpose(1, 0, 2)).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 3.5 composition
def gemm(A, lda, Bm, ldb, D, ldd, I, J, K, epi, bias=None, scale=None, res=None, ldr=0):
    _lib.call("gp_gemm_kmajor", _lib.ptr(A), _lib.i(lda), _lib.ptr(Bm), _lib.i(ldb), _lib.ptr(D), _lib.i(ldd), _lib.i(I), _lib.i(J), _lib.i(K),
              _lib.i(epi), _lib.ptr(bias), _lib.ptr(scale), _lib.ptr(res), _lib.i(ldr), _lib.stream_ptr())


@pytest.mark.parametrize("dim", [128, 384])
def test_one_block_composed_from_the_stage_entries_equals_the_product_forward(dim):
    """One block of the chain ViT on the PRODUCT library (B = 3, stop_after_layers = 1, normalize = 0) against the same block rebuilt from
    the embedding with stage calls in the forward's order and buffers: gp_vit_layernorm_f32 -> gp_gemm_kmajor (q | k: epilogue 1, v:
    epilogue 4) -> gp_vit_attention_f32 -> gp_gemm_kmajor epilogue 3; gp_vit_layernorm_f32 -> epilogue 2 -> epilogue 3 -> gp_vit_features.
    The f32 stage entries run on the probe library, the GEMMs on the product library (gp_gemm_kmajor and the forward's stream-K launch
    are held bit-identical by test_gemm_streamk_is_bit_identical).  Bit-equal: any difference is a layout or dispatch difference between
    the entries and the forward, or between the two binaries' kernels."""
    B, H, mlp = 3, dim // 64, 4 * dim
    M, Mpad = B * 257, round_up(B * 257, 256)
    vit = make_vit(dim, 2, 41)
    x = torch.from_numpy(np.random.RandomState(42).standard_normal((B, 3, 224, 224)).astype(np.float32)).to(DEV)
    _, X = forward_with_nan_workspace(vit, x, 0)                   # the embedding of 3.4, [dim][Mpad] on the device
    want_out, want_X = forward_with_nan_workspace(vit, x, 1)
    assert not torch.equal(bits(X), bits(want_X))
    w = vit._packed[1][4:4 + 16]
    ln1_g, ln1_b, qk_wt, qk_b, v_wt, v_b, proj_wt, proj_b, ls1, ln2_g, ln2_b, fc1_wt, fc1_b, fc2_wt, fc2_b, ls2 = w
    Hn = torch.full((dim, Mpad), NAN, device=DEV)
    QK = torch.full((2 * dim, Mpad), NAN, device=DEV)
    Vt = torch.full((Mpad, dim), NAN, device=DEV)
    Fb = torch.full((mlp, Mpad), NAN, device=DEV)
    out = torch.full((B, dim, 256), NAN, device=DEV)
    st = _lib.stream_ptr()

    def stage(name, *args):
        with _lib.probe_library():
            _lib.call(name, *args)

    stage("gp_vit_layernorm_f32", _lib.ptr(X), _lib.ptr(Hn), _lib.ptr(ln1_g), _lib.ptr(ln1_b), _lib.i(dim), _lib.i(Mpad), _lib.f(EPS), st)
    gemm(qk_wt, 2 * dim, Hn, Mpad, QK, Mpad, 2 * dim, Mpad, dim, 1, qk_b)
    gemm(Hn, Mpad, v_wt, dim, Vt, dim, Mpad, dim, dim, 4, v_b)
    stage("gp_vit_attention_f32", _lib.ptr(QK), _lib.ptr(Vt), _lib.ptr(Hn), _lib.i(B), _lib.i(H), _lib.i(dim), _lib.i(Mpad), st)   # over the LN output, as the forward
    gemm(proj_wt, dim, Hn, Mpad, X, Mpad, dim, Mpad, dim, 3, proj_b, ls1, X, Mpad)
    stage("gp_vit_layernorm_f32", _lib.ptr(X), _lib.ptr(Hn), _lib.ptr(ln2_g), _lib.ptr(ln2_b), _lib.i(dim), _lib.i(Mpad), _lib.f(EPS), st)
    gemm(fc1_wt, mlp, Hn, Mpad, Fb, Mpad, mlp, Mpad, dim, 2, fc1_b)
    gemm(fc2_wt, dim, Fb, Mpad, X, Mpad, dim, Mpad, mlp, 3, fc2_b, ls2, X, Mpad)
    stage("gp_vit_features", _lib.ptr(X), _lib.ptr(out), _lib.i(B), _lib.i(dim), _lib.i(Mpad), _lib.i(0), st)
    torch.cuda.synchronize()
    _lib.check_status()
    assert bool(torch.isfinite(X).all()) and bool(torch.isfinite(out).all())
    nx = int((bits(X[:, :M]) != bits(want_X[:, :M])).sum())
    npad = int((bits(X[:, M:]) != bits(want_X[:, M:])).sum())
    no = int((bits(out.cpu()) != bits(want_out)).sum())
    print(f"composition dim={dim}: {nx} of {dim * M} token elements, {npad} pad elements of x_prenorm^T and {no} feature elements differ from the product forward")
    assert nx == 0 and npad == 0 and no == 0
