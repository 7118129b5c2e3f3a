"""Input builders and float64 references of the stage tests of the split path's non-GEMM kernels (tests/test_gpu_layernorm_planes.py,
test_gpu_ist_split.py, test_gpu_stem_planes.py, test_gpu_plane_producers.py) and of the f32 ViT kernels behind the plane path
(tests/test_gpu_vit_f32_stages.py).  numpy / torch on the CPU only: nothing here touches a GPU or
the HIP library, and tests/test_stage_refs.py checks every function of this file against torch's own float64 operators without one.

Conventions restated (include/gigapose_hip.h):
  * activation planes: hi = f16(s x), lo = f16(s x - hi), round-to-nearest-even, s = 8 unless said otherwise; value = (hi + lo) / s;
  * LayerNorm -> planes: X [C][Mpad] f32 channel-major in, planes [Mpad][C] out (HF modeling_dinov2.py:342-380 norm1 / norm2);
  * the split stem: resized crops as 4-channel planes (B, S + 6, S + 8, 4) inside a frame of zeros, weights (Cout, 224) with
    k = dy * 32 + dx * 4 + ci (zeros at dx = 7 and ci = 3), stride 2, no padding = Conv2d(3 -> Cout, 7 x 7, stride 2, padding 3);
  * the IST regressor: rows (b, j, t) of (B, k, 256) whose four point coordinates are all != -1 are live, every other row is -1000.
"""
import numpy as np
import torch

P = 256
G = 16
PLANE_BITS = 2.0 ** -22          # hi + lo carry 22 bits of s x


# ---------------------------------------------------------------------------------------------------------------- planes
def split_planes_host(x, scale):
    """v = f32(s * x); hi = f16(v); lo = f16(v - f32(hi)) -- every step one IEEE operation in round-to-nearest-even (torch CPU)."""
    x = torch.as_tensor(x, dtype=torch.float32)
    v = x * torch.tensor(float(scale), dtype=torch.float32)
    hi = v.to(torch.float16)
    lo = (v - hi.to(torch.float32)).to(torch.float16)
    return hi, lo


def planes_value(hi, lo, scale):
    """float64 value a plane pair holds."""
    return (hi.double() + lo.double()) / float(scale)


def f16_ulp(h):
    """Spacing of f16 at |h| (float64 tensor): 2^(e - 10) for normal numbers, 2^-24 below 2^-14."""
    a = h.double().abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10.0)


def planes_well_formed(hi, lo):
    """|lo| <= ulp(hi) / 2 (a tie allowed) and everything finite."""
    ok = torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()
    return bool(ok) and bool((lo.double().abs() <= 0.5 * f16_ulp(hi)).all())


def split_values_case(count, seed):
    """f32 values for the bit-exact plane tests: magnitudes 1e-30 .. 8000 of both signs and, from the front (as far as `count`
    allows), +-0, exact f16 values (lo = 0), halfway cases of the f16 rounding, values whose lo plane is an f16 subnormal."""
    rs = np.random.RandomState(seed)
    x = (10.0 ** rs.uniform(-30.0, np.log10(8000.0), count) * rs.choice([-1.0, 1.0], count)).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -2.5, 0.333251953125, 1024.0, 4096.0,          # zeros, exact f16 values
                        1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, -(2.0 + 2.0 ** -10), 1000.25,   # ties of the hi rounding
                        1.0 + 2.0 ** -11 + 2.0 ** -22, 1.0 + 2.0 ** -11 - 2.0 ** -22,              # just beside a tie
                        1.0 + 2.0 ** -20, -(0.5 + 2.0 ** -23), 3.0 + 2.0 ** -22,                     # lo = a few 2^-24: f16 subnormals
                        2.0 ** -16, 3.0 * 2.0 ** -26, 6.0e-8, 1.0e-30, 8000.0, -7999.5], np.float32)
    if count >= 2:
        n = min(count - 1, len(special))      # x[0] stays a generic value when count == 1 is asked for on its own
        x[1:1 + n] = special[:n]
    return x


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_CLASSES = ("plain", "massive", "offset", "constant", "pad")
LN_MASSIVE = ((7, 250.0), (-3, -180.0))     # (channel, added value): channel 7 and channel C - 3


def layernorm_class_columns(Mpad):
    """Token columns of every special class: the first and the last column of 16 / 32 / 64-token blocks, columns in the middle of a
    block, the last columns of the buffer, and one column in 37 all along it (every lane of a block is met).  Every other column is
    `plain`; the pad columns sit at the end as in the residual stream."""
    fixed = {"massive": [0, 15, 64, 95, 127, 1000, Mpad // 2 + 31, Mpad - 4],
             "offset": [16, 31, 63, 128, 191, 1001, Mpad // 2 + 32, Mpad - 3],
             "constant": [32, 47, 192, 255, 256, 1002, Mpad // 2 + 63, Mpad - 2],
             "pad": [Mpad - 8, Mpad - 7, Mpad - 6, Mpad - 5, Mpad - 1]}
    fixed = {name: [c for c in cc if c < Mpad] for name, cc in fixed.items()}     # Mpad = 512: the columns near 1000 do not exist
    taken = {c for cc in fixed.values() for c in cc}
    for name, r in (("massive", 5), ("offset", 11), ("constant", 17)):
        fixed[name] = fixed[name] + [c for c in range(r, Mpad - 8, 37) if c not in taken]
    return fixed


def layernorm_case(C, Mpad, seed):
    """-> x [Mpad][C] f32 (token-major; the kernel reads its transpose), cls [Mpad] (index into LN_CLASSES), gamma, beta.
    plain: N(0,1) x a per-token scale in [0.3, 3] + a per-channel offset 0.5 N(0,1); massive: plain + 250 on one channel, - 180 on
    another; offset: plain + 50 everywhere; constant: 3.0 everywhere; pad: zeros.  gamma in +-[0.2, 2], beta N(0,1)."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((Mpad, C)) * rs.uniform(0.3, 3.0, (Mpad, 1)) + 0.5 * rs.standard_normal((1, C))
    cls = np.zeros(Mpad, np.int64)
    for name, cols in layernorm_class_columns(Mpad).items():
        cls[cols] = LN_CLASSES.index(name)
    for ch, add in LN_MASSIVE:
        x[cls == 1, ch] += add
    x[cls == 2] += 50.0
    x[cls == 3] = 3.0
    x[cls == 4] = 0.0
    gamma = rs.uniform(0.2, 2.0, C) * rs.choice([-1.0, 1.0], C)
    beta = rs.standard_normal(C)
    return (torch.from_numpy(x.astype(np.float32)), torch.from_numpy(cls), torch.from_numpy(gamma.astype(np.float32)),
            torch.from_numpy(beta.astype(np.float32)))


def layernorm_f64(x, gamma, beta, eps):
    """y = (x - mean) / sqrt(var + eps) * gamma + beta over the last axis in float64 on the f32 inputs (var = the biased one,
    mean((x - mean)^2), as torch.nn.LayerNorm).  Returns (y, xhat)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    xhat = d / torch.sqrt(var + eps)
    return xhat * gamma + beta, xhat


def layernorm_error(val, y64, xhat, gamma, beta):
    """e = |val - y64| / (|gamma| (|xhat| + 1) + |beta|), elementwise [M][C] float64."""
    return (val.double() - y64).abs() / (gamma.double().abs() * (xhat.abs() + 1.0) + beta.double().abs())


def per_class_max(e, cls):
    """{class name: max of e over the tokens of the class} for the classes present."""
    return {name: float(e[cls == i].max()) for i, name in enumerate(LN_CLASSES) if bool((cls == i).any())}


def layernorm_partial_sums_f32(x, gamma, beta, eps, slices, contiguous=False):
    """numpy f32 model of the kernels' documented summation order: `slices` (16 or 32) partial sums per token, each a sequential f32 sum
    over the slice's channels -- channels 8 sl + e of every chunk of 8 * slices channels (layernorm_planes_reg_kernel), or with
    `contiguous` the C / slices channels from sl C / slices on (layernorm_planes_kernel) -- added up in slice order; two passes
    (mean, then sum of fma(d, d, .)); y = (x - mean) * rstd * gamma + beta in f32.  x [M][C] f32 -> y [M][C] f32."""
    x = np.asarray(x, np.float32)
    M, C = x.shape
    ch = 8 * slices
    if contiguous:
        xs = x.reshape(M, slices, C // slices)
    else:
        xs = x.reshape(M, C // ch, slices, 8).transpose(0, 2, 1, 3).reshape(M, slices, C // slices)

    def seq_sum(v):      # sequential f32 sum over the last axis
        acc = np.zeros(v.shape[:-1], np.float32)
        for i in range(v.shape[-1]):
            acc = (acc + v[..., i]).astype(np.float32)
        return acc

    mean = (seq_sum(seq_sum(xs)) / np.float32(C)).astype(np.float32)
    d = (xs - mean[:, None, None]).astype(np.float32)
    q = np.zeros((M, slices), np.float32)
    for i in range(d.shape[-1]):     # fma(d, d, q): one rounding
        q = (d[..., i].astype(np.float64) * d[..., i].astype(np.float64) + q.astype(np.float64)).astype(np.float32)
    var = (seq_sum(q) / np.float32(C)).astype(np.float32)
    rstd = (np.float32(1.0) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    g, b = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    y = ((x - mean[:, None]).astype(np.float32) * rstd[:, None]).astype(np.float32)
    return ((y * g).astype(np.float32) + b).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the split stem
def pack_stem_weights(w):
    """(Cout, 3, 7, 7) -> (Cout, 224) with k = dy * 32 + dx * 4 + ci over a kernel row of 8 taps x 4 channels; dx = 7 and ci = 3 are
    zeros.  (The GPU tests take the packed planes from ResNet._pack_planes; this restatement serves the reference's own test.)"""
    w = torch.as_tensor(w)
    ws = torch.zeros(w.shape[0], 7, 8, 4, dtype=w.dtype)
    ws[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    return ws.reshape(w.shape[0], 224)


def frame_image(x):
    """(B, 3, S, S) -> the zero frame (B, S + 6, S + 8, 4): image at rows / columns 3 .. S + 2, channels 0 .. 2."""
    B, _, S, _ = x.shape
    f = torch.zeros(B, S + 6, S + 8, 4, dtype=x.dtype)
    f[:, 3:S + 3, 3:S + 3, :3] = x.permute(0, 2, 3, 1)
    return f


def stem_conv_framed_f64(frame, wk):
    """frame (B, S + 6, S + 8, 4), wk (Cout, 224), k = dy * 32 + dx * 4 + ci -> (B, Cout, S / 2, S / 2) float64: stride 2, no padding,
    output pixel (oy, ox) reads frame rows 2 oy .. 2 oy + 6 and columns 2 ox .. 2 ox + 7."""
    frame, wk = frame.double(), wk.double()
    B, Hp, Wp, _ = frame.shape
    S = Hp - 6
    assert Wp == S + 8 and wk.shape[1] == 224 and S % 2 == 0
    w = wk.reshape(-1, 7, 8, 4).permute(0, 3, 1, 2)                       # (Cout, ci, dy, dx)
    y = torch.nn.functional.conv2d(frame.permute(0, 3, 1, 2), w, stride=2)    # (B, Cout, S / 2, S / 2 + 1)
    return y[:, :, :, :S // 2]


def bn_relu_f64(y, alpha, beta, relu):
    if alpha is not None:
        y = y * alpha.double()[None, :, None, None] + beta.double()[None, :, None, None]
    return torch.relu(y) if relu else y


def resize_f64(x, S):
    return torch.nn.functional.interpolate(x.double(), (S, S), mode="bilinear", align_corners=True)


# ---------------------------------------------------------------------------------------------------------------- IST regressor
def ist_regressor_f64(feats, weights, use_tanh=True):
    """feats [n][2D] float64, weights = {"scale" | "inplane": [W1, b1, W2, b2, W3, b3]} in torch's [out][in] layout (ist_net.py:
    140-155) -> scale [n], cos_sin [n][2] float64."""
    outs = []
    for name in ("scale", "inplane"):
        W1, b1, W2, b2, W3, b3 = [torch.as_tensor(w).double() for w in weights[name]]
        h = torch.relu(feats @ W1.t() + b1)
        h = torch.relu(h @ W2.t() + b2)
        o = h @ W3.t() + b3
        outs.append(torch.tanh(o) if (use_tanh and name == "inplane") else o)
    return outs[0][:, 0], outs[1]


def ist_gather_f64(tar_feat, bank, labels0, id_src, tar_pts, src_pts, rows):
    """cat([tar, src]) features (batch.py:46-73, index = y * 16 + x) of the flat rows `rows` of (B, k, 256) -> [n][2D] float64."""
    B, k = id_src.shape
    D = tar_feat.shape[1]
    tf = torch.as_tensor(tar_feat).double().reshape(B, D, P)
    bk = torch.as_tensor(bank).double().reshape(bank.shape[0], bank.shape[1], D, P)
    rows = np.asarray(rows)
    b, j = rows // (k * P), (rows // P) % k
    tp = np.asarray(tar_pts).reshape(-1, 2)[rows]
    sp = np.asarray(src_pts).reshape(-1, 2)[rows]
    ti, si = tp[:, 1] * G + tp[:, 0], sp[:, 1] * G + sp[:, 0]
    obj, view = np.asarray(labels0)[b], np.asarray(id_src)[b, j]
    b, ti, si, obj, view = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)) for v in (b, ti, si, obj, view))
    return torch.cat([tf[b, :, ti], bk[obj, view, :, si]], dim=1)


IST_LIVE_COUNTS = (0, 1, 127, 128, 129, 1280, 1281, 3071, 3072)      # of R = 4 * 3 * 256 = 3072 rows = 24 column tiles of 128


def ist_points_case(seed, B, k):
    """Fully specified points for all R = B k 256 rows (tar = the patch's own grid position, src random) and an order of the rows
    whose first entry lies in the last (b, j) block: the set with n live rows keeps the first n rows of that order, so the sets are
    nested and a row that is live in two sets has the same points in both."""
    rs = np.random.RandomState(seed)
    R = B * k * P
    t = np.arange(P)
    tar = np.broadcast_to(np.stack([t % G, t // G], -1), (B, k, P, 2)).astype(np.int64).copy()
    src = rs.randint(0, G, (B, k, P, 2)).astype(np.int64)
    order = rs.permutation(R)
    first = int(np.nonzero(order >= R - P)[0][0])
    order[[0, first]] = order[[first, 0]]
    return tar, src, order


def ist_live_set(tar, src, order, n_live):
    """-> (tar_pts, src_pts, live): the rows order[:n_live] keep their points, every other row is (-1, -1) on both sides."""
    R = order.shape[0]
    live = np.zeros(R, bool)
    live[order[:n_live]] = True
    tp, sp = tar.reshape(R, 2).copy(), src.reshape(R, 2).copy()
    tp[~live] = -1
    sp[~live] = -1
    return tp.reshape(tar.shape), sp.reshape(src.shape), live


def ist_half_specified(tar_pts, src_pts, live, seed, n=64):
    """Turns n dead rows into half-specified ones -- x = -1 with y set, or y = -1 with x set, on the tar side, the src side or both,
    the other side fully specified -- which the reference counts as invalid (ist_net.py:109-119).  Returns new arrays + the rows."""
    rs = np.random.RandomState(seed)
    R = live.shape[0]
    tp, sp = tar_pts.reshape(R, 2).copy(), src_pts.reshape(R, 2).copy()
    rows = rs.choice(np.nonzero(~live)[0], n, replace=False)
    for i, r in enumerate(rows):
        tp[r] = rs.randint(0, G, 2)
        sp[r] = rs.randint(0, G, 2)
        kind = i % 6
        if kind == 0:
            tp[r, 0] = -1
        elif kind == 1:
            tp[r, 1] = -1
        elif kind == 2:
            sp[r, 0] = -1
        elif kind == 3:
            sp[r, 1] = -1
        elif kind == 4:
            tp[r, 0], sp[r, 1] = -1, -1
        else:
            tp[r, 1], sp[r, 0] = -1, -1
    return tp.reshape(tar_pts.shape), sp.reshape(src_pts.shape), rows


# ---------------------------------------------------------------------------------------------------------------- split attention
T_TOK = 257                      # tokens per crop: cls + 256 patches
ATTN_CHUNKS = ((0, 96), (96, 192), (192, 257))     # attention_split_kernel's three passes over the keys (the last one holds 65 + 31 masked)
ATTN_CLASSES = ("plain", "peaked", "sink", "sink256", "offset", "uniform", "zero_q", "descending", "ascending")
ATTN_OTHER_SCALE = ("plain", "peaked", "offset")   # the classes that also run on planes that carry another scale than 8


def attention_case(cls, B, H, seed):
    """-> q | k | v as one f32 tensor [B * 257][3 * 64 H] (the layout gp_attention_split reads, before the split into planes).
    Base: N(0, 1) everywhere.  d = a random unit vector of the 64 head channels (one per case).
      plain       q, k x 1.5                                       logit std 2-3 (the only kind of input the stage tests had)
      peaked      q, k x 4                                          softmax close to one-hot
      sink        q += 6 d, k[0] += 30 d, k[256] += 30 d            two keys (the first and the LAST) take nearly all the weight
      sink256     q += 6 d, k[256] += 30 d                          the one valid key of the masked last tile takes it
      offset      channel 7 of q = 40 + 0.1 n, of k = 60 + 0.1 n    logits near 300 with an ordinary spread: the f32 rounding of the logit
      uniform     every key of an image = its key 0                 softmax = 1 / 257 exactly: the output is the column mean of V
      zero_q      q = 0                                             the same through zero logits
      descending  q += 8 d, k[:96] += 12 d, k[96:] -= 12 d          the maximum sits in chunk 0, > 15 log2 units above the later chunks
      ascending   q += 8 d, k[:192] -= 12 d, k[192:] += 12 d        ... in the last chunk: the running reference jumps, alpha ~ 0"""
    assert cls in ATTN_CLASSES
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T_TOK, H, 64, generator=g, dtype=torch.float64) for _ in range(3))
    d = torch.randn(64, generator=g, dtype=torch.float64)
    d = d / d.norm()
    n1, n2 = (torch.randn(B, T_TOK, H, generator=g, dtype=torch.float64) for _ in range(2))
    if cls == "plain":
        q, k = 1.5 * q, 1.5 * k
    elif cls == "peaked":
        q, k = 4.0 * q, 4.0 * k
    elif cls in ("sink", "sink256"):
        q = q + 6.0 * d
        k[:, 256] += 30.0 * d
        if cls == "sink":
            k[:, 0] += 30.0 * d
    elif cls == "offset":
        q[..., 7] = 40.0 + 0.1 * n1
        k[..., 7] = 60.0 + 0.1 * n2
    elif cls == "uniform":
        k = k[:, :1].expand(B, T_TOK, H, 64).clone()
    elif cls == "zero_q":
        q = torch.zeros_like(q)
    elif cls == "descending":
        q = q + 8.0 * d
        k[:, :96] += 12.0 * d
        k[:, 96:] -= 12.0 * d
    elif cls == "ascending":
        q = q + 8.0 * d
        k[:, :192] -= 12.0 * d
        k[:, 192:] += 12.0 * d
    return torch.stack([q, k, v], dim=2).reshape(B * T_TOK, 3 * 64 * H).float()


def attention_qkv(vals, B, H):
    """[B * 257][3 * 64 H] values (any float type) -> q, k, v [B][H][257][64]."""
    x = vals.reshape(B, T_TOK, 3, H, 64)
    return x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)


def attention_logits(vals, B, H):
    """float64 logits q . k / 8 [B][H][query][key] (HF modeling_dinov2.py:207-229, head width 64)."""
    q, k, _ = attention_qkv(vals.double(), B, H)
    return q @ k.transpose(-1, -2) * 0.125


def attention_ref(vals, B, H, dtype=torch.float64):
    """softmax(q k^T / 8) v evaluated in `dtype` on the given values -> [B][257][H][64] (the layout of the output planes).
    float64: the reference.  float32: torch's own f32 evaluation of the same formula (one rounding of the scaled logit, as the kernel has),
    whose error against float64 sets the kernel's bound."""
    q, k, v = attention_qkv(vals.to(dtype), B, H)
    return (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).permute(0, 2, 1, 3)


def attention_preconditions(cls, logits, vals=None, B=None, H=None):
    """{name: (figure, holds)} of the class on its float64 logits [B][H][257][257]: what makes the case the edge it is named after.
    A generator that stops producing the edge fails here, not silently in front of the kernel."""
    p = torch.softmax(logits, dim=-1)
    ent = -(p * torch.log(p.clamp_min(1e-300))).sum(-1)
    out = {}
    if cls == "plain":
        s = float(logits.std())
        out["logit std in [2, 3]"] = (s, 2.0 <= s <= 3.0)
    elif cls == "peaked":
        out["mean entropy < 0.5"] = (float(ent.mean()), float(ent.mean()) < 0.5)
        out["logit std > 10"] = (float(logits.std()), float(logits.std()) > 10.0)
    elif cls == "sink":
        top = float(p.max(-1).values.mean())
        out["mean top weight > 0.7"] = (top, top > 0.7)
        frac = float(((p[..., 0] + p[..., 256]) > 0.99).double().mean())
        out["keys 0 + 256 hold > 0.99 of the weight in > 99 % of rows"] = (frac, frac > 0.99)
        first = float((logits.argmax(-1) == 0).double().mean())
        out["key 0 leads in 30-70 % of rows, key 256 in the others"] = (first, 0.3 <= first <= 0.7)
    elif cls == "sink256":
        frac = float((logits.argmax(-1) == 256).double().mean())
        out["argmax key = 256 in > 99 % of rows"] = (frac, frac > 0.99)
        f256 = float((logits[:, :, 256].argmax(-1) == 256).double().mean())
        out["... and for every query 256"] = (f256, f256 == 1.0)
    elif cls == "offset":
        out["max |logit| > 250"] = (float(logits.abs().max()), float(logits.abs().max()) > 250.0)
        out["mean entropy > 4.5"] = (float(ent.mean()), float(ent.mean()) > 4.5)
    elif cls in ("uniform", "zero_q"):
        spread = float((logits.max(-1).values - logits.min(-1).values).max())
        out["logits of a row all equal (to float64 round-off of the 64-term dot products)"] = (spread, spread <= 1e-12)
    else:
        LOG2E = 1.4426950408889634
        cm = torch.stack([logits[..., a:b].max(-1).values for a, b in ATTN_CHUNKS], dim=-1) * LOG2E      # chunk maxima, log2 units
        lead = 0 if cls == "descending" else 2
        others = [c for c in range(3) if c != lead]
        gap = cm[..., lead] - torch.maximum(cm[..., others[0]], cm[..., others[1]])
        frac = float((gap > 15.0).double().mean())
        out[f"chunk {lead} maximum > 15 log2 units above both others in >= 99 % of rows (minimum gap {float(gap.min()):.1f})"] = (frac, frac >= 0.99)
    return out


# deliberately wrong attention "references" (tests/test_stage_refs.py shows that the float64 reference tells each from the right one by far
# more than the bound the kernel is held to -- every one is a bug attention_split_kernel could have)
def attention_mutant(kind, vals, B, H):
    q, k, v = attention_qkv(vals.double(), B, H)
    if kind == "drop_key_256":            # wave 0 forgets key 256 / the last tile is masked one key too early
        return (torch.softmax(q @ k[:, :, :256].transpose(-1, -2) * 0.125, dim=-1) @ v[:, :, :256]).permute(0, 2, 1, 3)
    if kind == "scale_63":                # 1 / sqrt(63) instead of 1 / 8
        return (torch.softmax(q @ k.transpose(-1, -2) * 63.0 ** -0.5, dim=-1) @ v).permute(0, 2, 1, 3)
    if kind == "per_chunk_max":           # every chunk relative to its OWN maximum, no alpha rescale of what came before
        s = q @ k.transpose(-1, -2) * 0.125
        num, den = 0.0, 0.0
        for a, b in ATTN_CHUNKS:
            pc = torch.exp(s[..., a:b] - s[..., a:b].max(-1, keepdim=True).values)
            num, den = num + pc @ v[:, :, a:b], den + pc.sum(-1, keepdim=True)
        return (num / den).permute(0, 2, 1, 3)
    # ---- bugs attention_body (the f32 kernel: one wave per 32 queries, a lane half per 16 keys of a 32-key tile) could have
    if kind == "half_denominator":        # l_part without its cross-half share: the denominator holds the keys of lane half 0 only
        p = torch.exp(q @ k.transpose(-1, -2) * 0.125 - (q @ k.transpose(-1, -2) * 0.125).max(-1, keepdim=True).values)
        return ((p @ v) / p[..., attention_half_keys(0)].sum(-1, keepdim=True)).permute(0, 2, 1, 3)
    if kind == "channel_halves_swapped":  # o0 / o1 stored to each other's rows: channels d and 32 + d of a head exchanged
        return torch.roll(attention_ref(vals, B, H), 32, dims=-1)
    if kind == "query_256_from_next_crop":   # a crop stride of 256 on the q side of the last query tile: crop b reads crop b + 1's q
        q = q.clone()
        q[:, :, 256] = torch.roll(q[:, :, 256], -1, dims=0)
        return (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).permute(0, 2, 1, 3)
    raise ValueError(kind)


ATTN_MUTANTS = ("drop_key_256", "scale_63", "per_chunk_max", "half_denominator", "channel_halves_swapped", "query_256_from_next_crop")


def attention_half_keys(half):
    """The keys whose P registers lane half `half` of attention_body holds: in every 32-key tile rows frag_row(r, lane) =
    (r & 3) + 8 (r >> 2) + 4 half, r = 0 .. 15 (gp_common.h) -- the keys with (key % 8) // 4 == half; only keys < 257 exist."""
    return torch.tensor([t for t in range(T_TOK) if (t % 8) // 4 == half])


def attention_cm_layout(vals, B, H, Mpad, fill):
    """[B * 257][3 * 64 H] values of attention_case -> (qk [2 * 64 H][Mpad], vt [Mpad][64 H]) f32 as gp_vit_attention_f32 reads them: Q in
    rows h * 64 + d, K in rows 64 H + h * 64 + d, column = token b * 257 + t; V token-major.  Pad columns of qk and pad rows of vt = fill."""
    C, M = 64 * H, B * T_TOK
    assert vals.shape == (M, 3 * C) and Mpad >= M
    qk = torch.full((2 * C, Mpad), float(fill), dtype=torch.float32)
    vt = torch.full((Mpad, C), float(fill), dtype=torch.float32)
    qk[:, :M] = vals[:, :2 * C].t().float()
    vt[:M] = vals[:, 2 * C:].float()
    return qk, vt


def attention_cm_values(qk, vt, B, H):
    """Inverse of attention_cm_layout on the token columns: -> [B * 257][3 * 64 H]."""
    M = B * T_TOK
    return torch.cat([qk[:, :M].t(), vt[:M]], dim=1)


def attention_cm_output(out, B, H):
    """out [64 H][Mpad] channel-major (gp_vit_attention_f32) -> [B][257][H][64], the layout of attention_ref."""
    return out[:, :B * T_TOK].t().reshape(B, T_TOK, H, 64)


def attention_cm_from_output(o, Mpad, fill):
    """Inverse of attention_cm_output: [B][257][H][64] -> [64 H][Mpad] f32, pad columns = fill."""
    B, _, H, _ = o.shape
    out = torch.full((64 * H, Mpad), float(fill), dtype=torch.float32)
    out[:, :B * T_TOK] = o.reshape(B * T_TOK, 64 * H).t().float()
    return out


def attention_bound_f32(e32):
    """Bound of the f32 kernel (attention_kernel, f32 in and out: no plane term) on max |err| / max |ref|: twice torch's own f32 evaluation
    of the formula on the same values (another summation order and nothing else), not below 2e-6 -- the floor its f16-plane twin is
    held to on x 8 planes; the f32 kernel may not be worse."""
    return max(2.0 * e32, 2e-6)


def attention_bound(e32, scale):
    """The kernel's bound on max |err| / max |ref|: twice torch's own f32 evaluation of the formula on the same values (a different
    summation order and nothing else), not below the stage bound the kernel already had (2e-6 on x 8 planes, 4e-6 on others), plus the
    output planes' 22 bits."""
    return max(2.0 * e32, 2e-6 if scale == 8.0 else 4e-6) + 2.0 ** -21


# ---------------------------------------------------------------------------------------------------------------- the split matcher
# match_tiles_split_kernel (gp_match.hip) against float64 at every live-block layout: input builders, the float64 restatement of the
# reference matcher on the values the kernel reads (matching.py:233-278 with find_consistency_patches :80-113), and a checker in the
# manner of tests/parity_explain.py -- a difference from the float64 run is legitimate only where it sits on a float64 decision margin.
MATCH_SCALE = 32.0                                   # the matcher's planes hold 32 x the unit vectors (kFeatScale)
MATCH_COUNTS_X = (0, 1, 33, 65, 97, 129, 161, 193, 225)      # live patches per row: ceil(c / 32) = 0 .. 8
MATCH_COUNTS_Y = (0, 32, 64, 96, 128, 160, 192, 224, 256)
MATCH_DUP_TMPL = (7, 200)                            # template patch 200 is a copy of patch 7 (row ties)
MATCH_DUP_QUERY = (11, 250)                          # query patch 250 is a copy of patch 11 (column ties across row groups)
MATCH_FRAC_ROWS = (5, 6)                             # the query row / the template row whose live mask values are fractional
MATCH_NEAR = 4e-6                                    # the fixed distance of the precondition "few decisions sit on a margin"
MATCH_EXCUSED_CAP = 0.005                            # at most 0.5 % of the checked entries may be excused
MATCH_O3_LABELS = (2, 0, 1, 2, 2, 0, 1, 0, 2)


def _unit_rows(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def match_live_masks(counts, seed, frac_row=None, keep=()):
    """(len(counts), 256) f32 masks with exactly counts[r] live patches in row r at seeded positions.  Patches 0 (the "no match"
    sentinel) and 255 are live in odd rows and dead in even rows wherever the count allows; the patches `keep` are live wherever the
    count leaves room for them.  Row `frac_row` carries values in [0.75, 1) instead of 1."""
    rs = np.random.RandomState(seed)
    m = np.zeros((len(counts), P), np.float32)
    for r, c in enumerate(counts):
        order = rs.permutation(P)
        want_live = [p for p in (0, 255) if r % 2 == 1]
        want_dead = [p for p in (0, 255) if r % 2 == 0]
        live = []
        for p in want_live + list(keep):
            if len(live) < c and p not in live and p not in want_dead:
                live.append(p)
        dead = set(want_dead) if P - len(want_dead) >= c else set()
        for p in order:
            if len(live) >= c:
                break
            if p not in live and p not in dead:
                live.append(int(p))
        for p in order:                  # a full row: the forced-dead patches come last
            if len(live) >= c:
                break
            if p not in live:
                live.append(int(p))
        m[r, live] = 1.0
        if r == frac_row:
            m[r, live] = rs.uniform(0.75, 1.0, len(live)).astype(np.float32)
    return m


def match_blocks_case(which, C, seed=11, O=1, labels=None, anti=False, B=9, N=9):
    """The block cases of tests/test_gpu_matcher_f64.py.  which = "a": query rows with MATCH_COUNTS_X live patches, template rows with
    MATCH_COUNTS_Y; "b": the two sides exchanged -- every pair (ceil(live_t / 32), ceil(live_s / 32)) in 0..8 x 0..8 is a tile.
    Features: per object a base of 256 random unit vectors; template n = unit(base + tn[n] r), query b = unit(base[perm_b] + qn[b] r')
    with |r| ~ 1 and the noise levels spread so that the tile's similarity at a true match runs from ~0.95 to below the 0.5
    threshold; template patch 200 = patch 7 and query patch 250 = patch 11, bit for bit.  anti: every query close to one direction u
    and the templates 2, 5, 8 anti-correlated with it (similarities around -0.12, tests/test_gpu_matcher.py: _negative_case), for
    negative thresholds.  Returns f32 unit features q (B, 256, C), t (O, N, 256, C), masks qm (B, 256), tm (O, N, 256), labels (B,),
    and their x 32 planes (host split)."""
    rs = np.random.RandomState(seed + (0 if which == "a" else 1000) + C)
    qc, tc = (MATCH_COUNTS_X, MATCH_COUNTS_Y) if which == "a" else (MATCH_COUNTS_Y, MATCH_COUNTS_X)
    qc, tc = qc[:B], tc[:N]
    labels = np.zeros(B, np.int32) if labels is None else np.asarray(labels, np.int32)
    base = _unit_rows(rs.standard_normal((O, P, C)))
    tn, qn = rs.permutation(np.linspace(0.15, 1.1, N)), rs.permutation(np.linspace(0.15, 1.1, B))
    t = _unit_rows(base[:, None] + tn[None, :, None, None] * rs.standard_normal((O, N, P, C)) / np.sqrt(C))
    q = np.empty((B, P, C))
    for b in range(B):
        q[b] = _unit_rows(base[labels[b], rs.permutation(P)] + qn[b] * rs.standard_normal((P, C)) / np.sqrt(C))
    if anti:
        u = _unit_rows(rs.standard_normal(C))

        def around(mean, shape):
            v = rs.standard_normal(shape + (C,))
            v = _unit_rows(v - (v @ u)[..., None] * u)
            return mean * u + np.sqrt(1.0 - mean * mean) * v
        q = around(0.98, (B, P))
        for n in (2, 5, 8):
            if n < N:
                t[:, n] = around(-0.12, (O, P))
    q, t = q.astype(np.float32), t.astype(np.float32)
    t[:, :, MATCH_DUP_TMPL[1]] = t[:, :, MATCH_DUP_TMPL[0]]
    q[:, MATCH_DUP_QUERY[1]] = q[:, MATCH_DUP_QUERY[0]]
    qm = match_live_masks(qc, seed + 1, frac_row=MATCH_FRAC_ROWS[0], keep=MATCH_DUP_QUERY)
    tm = np.stack([match_live_masks(tc, seed + 2 + o, frac_row=MATCH_FRAC_ROWS[1], keep=MATCH_DUP_TMPL) for o in range(O)])
    case = dict(q=q, t=t, qm=qm, tm=tm, labels=labels, B=B, N=N, O=O, C=C)
    case["q_hi"], case["q_lo"] = split_planes_host(torch.from_numpy(q), MATCH_SCALE)
    case["b_hi"], case["b_lo"] = split_planes_host(torch.from_numpy(t), MATCH_SCALE)
    return case


def match_case_layouts(qm, tm, labels):
    """{(ceil(live_t / 32), ceil(live_s / 32))} over all tiles (b, n)."""
    lt = (np.asarray(qm) != 0).sum(-1)
    ls = (np.asarray(tm) != 0).sum(-1)
    return {(int(-(-lt[b] // 32)), int(-(-ls[labels[b], n] // 32))) for b in range(lt.shape[0]) for n in range(ls.shape[1])}


def match_value_coeff(q_hi, q_lo, b_hi, b_lo, labels, scale=MATCH_SCALE, tiles=None):
    """The value-error coefficient c of a case: 2 x the largest |e| / mag of torch's own float32 evaluation of the products the kernel
    forms -- hi hi + hi lo + lo hi (hi hi + lo hi for a one-plane bank; one f32 product for f32 features, q_lo = None) scaled by
    1 / scale^2 -- against the float64 product of the full values, mag = |q| |b|^T, over the tiles (b, n) given (default all).  The
    factor 2 covers another summation order.  Never derived from the kernel's output."""
    labels = np.asarray(labels)
    if tiles is None:
        tiles = [(b, n) for b in range(q_hi.shape[0]) for n in range(b_hi.shape[1])]
    inv = 1.0 / (scale * scale)
    worst = 0.0
    for b, n in tiles:
        o = int(labels[b])
        qh, bh = torch.as_tensor(q_hi[b]).cpu().float(), torch.as_tensor(b_hi[o, n]).cpu().float()
        ql = None if q_lo is None else torch.as_tensor(q_lo[b]).cpu().float()
        bl = None if b_lo is None else torch.as_tensor(b_lo[o, n]).cpu().float()
        s32 = qh @ bh.t()
        if bl is not None:
            s32 = s32 + qh @ bl.t()
        if ql is not None:
            s32 = s32 + ql @ bh.t()
        s32 = s32 * torch.tensor(inv, dtype=torch.float32)
        q64 = qh.double() + (0.0 if ql is None else ql.double())
        b64 = bh.double() + (0.0 if bl is None else bl.double())
        s64 = (q64 @ b64.t()) * inv
        mag = (q64.abs() @ b64.abs().t()) * inv
        worst = max(worst, float(((s32.double() - s64).abs() / mag.clamp_min(1e-300)).max()))
    return 2.0 * worst


def _first_of_identical_rows(x):
    """x (rows, K) -> for every row the index of the first row with the same bits."""
    x = np.ascontiguousarray(x)
    keys = x.view(np.uint8).reshape(x.shape[0], -1)
    first, out = {}, np.empty(x.shape[0], np.int64)
    for i in range(x.shape[0]):
        out[i] = first.setdefault(keys[i].tobytes(), i)
    return out


def _two_largest(T, axis):
    """first argmax, maximum and runner-up value (the maximum of the others) along `axis` of a 2-D array."""
    T = T if axis == 1 else T.T
    i = T.argmax(1)
    v = T[np.arange(T.shape[0]), i]
    rest = T.copy()
    rest[np.arange(T.shape[0]), i] = -np.inf
    return i, v, rest.max(1)


def _match_decisions(U, qm, sm, thr, patch_thr, src2tar, drop_rows=None):
    """One tile in float64.  U (256 t, 256 s): masked, unthresholded similarities.  Returns the reference's records and margins.
    drop_rows (mutant (c)): query patches whose values the column maxima do not see."""
    T = np.where(U < thr, 0.0, U)
    ri, rv, r2 = _two_largest(T, 1)
    Tc = T if drop_rows is None else np.where(drop_rows[:, None], -np.inf, T)
    ci, cv, c2 = _two_largest(Tc, 0)
    if drop_rows is not None:
        empty = ~np.isfinite(cv)
        cv, ci = np.where(empty, 0.0, cv), np.where(empty, 0, ci)
    ia, va, ib, vb = (ci, cv, ri, rv) if src2tar else (ri, rv, ci, cv)
    p = np.arange(P)
    js = ia
    ok = va >= thr
    if patch_thr > 0:
        t2 = ib[js]
        dist = np.sqrt(((t2 % G) - (p % G)).astype(np.float64) ** 2 + ((t2 // G) - (p // G)).astype(np.float64) ** 2)
        ok = ok & (dist <= patch_thr) & (vb[js] >= thr)
    nz = (qm.astype(np.float32) * sm.astype(np.float32)[js]) * (ib != 0).astype(np.float32) * (js != 0).astype(np.float32)
    mask = ok.astype(np.float32) * nz
    contrib = va * mask.astype(np.float64)
    avg = contrib.sum() / 256.0 if mask.sum() > 0 else 0.0
    return dict(idx=js, score=va, mask=mask, sim_avg=avg, row_i=ri, row_v=rv, row_2=r2, col_i=ci, col_v=cv, col_2=c2)


def match_tiles_f64(q_hi, q_lo, b_hi, b_lo, qmask, bmask, labels, thr, patch_thr, direction, scale=MATCH_SCALE, tiles=None,
                    _drop=None):
    """The reference matcher (matching.py:233-278, find_consistency_patches :80-113) in float64 on the values the kernel reads.
    q_hi / q_lo (B, 256, C), b_hi / b_lo (O, N, 256, C) planes (lo may be None: value = hi / scale), qmask (B, 256), bmask (O, N, 256),
    labels (B,) 0-based, direction "tar2src" | "src2tar"; tiles: the (b, n) to evaluate (default all, b-major).
    value = (hi + lo) / scale; sim = q b^T; sim *= both patch masks (fractional values multiply, :234-235); sim[sim < thr] = 0 (:236);
    row / column maxima, the first maximum wins (:240-241); src2tar exchanges the two (:242-244); mask_sim (:246), the cycle check
    with dist <= patch_thr (:249-255, skipped for patch_thr <= 0, :256-257), `idx_b != 0` read at POSITION p, `idx_a != 0`, the mask
    product (:258-266); sim_avg = sum(score * mask) / 256, 0 when no mask is set (:267-271).  Rows of a plane pair that are
    bit-identical give bit-identical similarities here too (the float64 product is formed once per distinct row).
    Returns a dict of arrays over the T tiles: idx, score, mask (f32 exactly as the f32 product of the mask values), sim_avg; U and
    mag (T, 256, 256) [t][s] = the masked unthresholded similarity and |q| |b|^T x |masks|; per row / column the first argmax, maximum
    and runner-up; row_margin / col_margin (best - runner-up), row_thr / col_thr (distance of the largest unthresholded value
    both masks keep from thr; inf where there is none); mag_at (T, 256) = mag at the chosen entries."""
    as64 = lambda x: None if x is None else torch.as_tensor(x).double().numpy()
    qh, ql, bh, bl = as64(q_hi), as64(q_lo), as64(b_hi), as64(b_lo)
    qv = (qh if ql is None else qh + ql) / scale
    bv = (bh if bl is None else bh + bl) / scale
    qmask, bmask, labels = np.asarray(qmask, np.float32), np.asarray(bmask, np.float32), np.asarray(labels)
    B, N = qv.shape[0], bv.shape[1]
    if tiles is None:
        tiles = [(b, n) for b in range(B) for n in range(N)]
    tiles = np.asarray(tiles, np.int64).reshape(-1, 2)
    src2tar = direction == "src2tar"
    assert direction in ("tar2src", "src2tar")
    keys = ["idx", "score", "mask", "sim_avg", "row_i", "row_v", "row_2", "col_i", "col_v", "col_2"]
    out = {k: [] for k in keys + ["U", "mag"]}
    for b, n in tiles:
        o = int(labels[b])
        q, t = qv[b], bv[o, n]
        fq, ft = _first_of_identical_rows(q), _first_of_identical_rows(t)
        S = (q @ t.T)[fq][:, ft]
        mm = qmask[b].astype(np.float64)[:, None] * bmask[o, n].astype(np.float64)[None, :]
        U = S * mm
        drop = None
        if _drop is not None:
            drop = _drop(qmask[b], bmask[o, n])
        d = _match_decisions(U, qmask[b], bmask[o, n], thr, patch_thr, src2tar, drop)
        for k in keys:
            out[k].append(d[k])
        out["U"].append(U)
        out["mag"].append((np.abs(q) @ np.abs(t).T) * np.abs(mm))
    out = {k: np.stack(v) if np.ndim(v[0]) else np.asarray(v) for k, v in out.items()}
    out["row_margin"], out["col_margin"] = out["row_v"] - out["row_2"], out["col_v"] - out["col_2"]
    live = np.where(out["mag"] > 0, out["U"], -np.inf)            # the entries both masks keep (a masked-out entry is an exact 0, no decision)
    out["row_live_max"], out["col_live_max"] = live.max(2), live.max(1)
    out["row_thr"], out["col_thr"] = np.abs(out["row_live_max"] - thr), np.abs(out["col_live_max"] - thr)
    ar = np.arange(P)
    ii = out["idx"]
    out["mag_at"] = np.stack([(m.T if src2tar else m)[ar, i] for m, i in zip(out["mag"], ii)])
    out.update(tiles=tiles, thr=float(thr), patch_thr=float(patch_thr), direction=direction, qm=qmask[tiles[:, 0]],
               sm=bmask[labels[tiles[:, 0]], tiles[:, 1]])
    return out


def match_ref_as_ours(ref, B, N):
    """The float64 records as a kernel would return them: idx u8, score / mask f32 (B, N, 256), sim_avg f32 (B, N)."""
    assert ref["tiles"].shape[0] == B * N
    return dict(idx=ref["idx"].reshape(B, N, P).astype(np.uint8), score=ref["score"].reshape(B, N, P).astype(np.float32),
                mask=ref["mask"].reshape(B, N, P).astype(np.float32), sim_avg=ref["sim_avg"].reshape(B, N).astype(np.float32))


def match_near_margin_share(ref, near=MATCH_NEAR):
    """Share of the row and column decisions of `ref` that sit within `near` of a margin: a runner-up (exact ties -- planted copies and
    all-zero rows -- excepted: they are decided by the index rule, not by a value) or the threshold."""
    close = 0
    total = 0
    for side in ("row", "col"):
        m, d = ref[side + "_margin"], ref[side + "_thr"]
        close += int((((m > 0) & (m <= near)) | (d <= near)).sum())
        total += m.size
    return close / max(total, 1)


class _Lazy:
    """A failure text that is formatted only when a failure is reported."""
    def __init__(self, fn):
        self.fn = fn

    def __radd__(self, other):
        return other + self.fn()

    def __add__(self, other):
        return self.fn() + other


def match_tiles_check(ours, ref, c):
    """ours: idx, score, mask (B, N, 256), sim_avg (B, N) (numpy) of the kernel; ref: match_tiles_f64's dict (its tiles are the ones
    checked); c: the value-error coefficient (match_value_coeff): the kernel's similarity may be off by c mag, so two values within
    eps = 2 c mag of each other may be ordered either way.  Per (b, n, p):
      * the index is the float64 first argmax of its row (column for src2tar); or its float64 value lies within eps of that maximum
        (EXCUSED); or the decision sits within eps of the threshold and the kernel returned (0, 0) / a value that close to the
        largest (EXCUSED).  An exact float64 tie -- planted copies, all-zero rows -- is never excused: the lower index must come back;
      * the score lies within c mag + 2^-23 |v| of the float64 value at the returned index (or is the exact 0 of a zeroed entry if
        that value is within the same distance of the threshold);
      * a row whose float64 maximum is more than eps below thr returns index 0 and score 0 exactly;
      * mask_all equals the float64 mask, unless a decision it depends on -- the row at p, the column at the matched index, the column
        at p, each against its runner-up and against the threshold -- is within eps of its margin (EXCUSED; exact ties are not);
      * sim_avg equals the float64 sum of the kernel's OWN score * mask / 256 to 256 * 2^-24 relative, and is exactly 0 when no mask is set.
    Returns dict(checked, excused, failed, max_ratio = max |score err| / bound, first = a readable first failure or None)."""
    tiles, thr, src2tar = ref["tiles"], ref["thr"], ref["direction"] == "src2tar"
    ar = np.arange(P)
    checked = excused = failed = 0
    max_ratio, first = 0.0, None

    def fail(msg):
        nonlocal failed, first
        failed += 1
        if first is None:
            first = msg
    for k, (b, n) in enumerate(tiles):
        U = ref["U"][k].T if src2tar else ref["U"][k]            # rows = the positions p of side A, columns = the matched index
        mag = ref["mag"][k].T if src2tar else ref["mag"][k]
        T = np.where(U < thr, 0.0, U)
        a_i, a_v, a_2 = (ref["col_i"][k], ref["col_v"][k], ref["col_2"][k]) if src2tar else (ref["row_i"][k], ref["row_v"][k], ref["row_2"][k])
        a_m, a_t = (ref["col_margin"][k], ref["col_thr"][k]) if src2tar else (ref["row_margin"][k], ref["row_thr"][k])
        b_m, b_t = (ref["row_margin"][k], ref["row_thr"][k]) if src2tar else (ref["col_margin"][k], ref["col_thr"][k])
        j = ours["idx"][b, n].astype(np.int64)
        sc = ours["score"][b, n].astype(np.float64)
        mk = ours["mask"][b, n]
        umax = U.max(1)
        lmax = ref["col_live_max"][k] if src2tar else ref["row_live_max"][k]
        mag_row = mag.max(1)
        eps_row = 2.0 * c * np.maximum(mag_row, 1e-300)
        idx_state = np.zeros(P, np.int8)       # 0 equal, 1 excused, 2 failed
        for p in ar:
            checked += 1
            jj, best = int(j[p]), int(a_i[p])
            eps = 2.0 * c * max(mag[p, jj], mag[p, best])
            where = _Lazy(lambda: f"det {b} template {n} patch {p}: ours idx {jj} score {sc[p]:.9g}; float64 best {best} ({a_v[p]:.12g}) "
                          f"runner-up {a_2[p]:.12g} margin {a_m[p]:.3g}, max - thr {umax[p] - thr:.3g}, eps {eps:.3g}")
            # the score at the returned index
            tol = c * mag[p, jj] + 2.0 ** -23 * abs(U[p, jj])
            err = abs(sc[p] - T[p, jj])
            if tol > 0:
                max_ratio = max(max_ratio, err / tol)
            near_thr_here = abs(U[p, jj] - thr) <= tol
            score_ok = err <= tol or (near_thr_here and (sc[p] == 0.0 or abs(sc[p] - U[p, jj]) <= tol))
            if not score_ok:
                fail("score: " + where + f"; float64 value at ours {T[p, jj]:.12g}, |err| {err:.3g} > bound {tol:.3g}")
                idx_state[p] = 2
                continue
            if umax[p] < thr - eps_row[p] and (jj != 0 or sc[p] != 0.0):
                fail("a row below the threshold must return (0, 0): " + where)
                idx_state[p] = 2
                continue
            if jj == best and (sc[p] != 0.0) == (a_v[p] != 0.0):
                continue
            tj = U[p, jj] if sc[p] != 0.0 else 0.0                  # the float64 value of what the kernel says it found
            d = a_v[p] - tj
            on_thr = abs(lmax[p] - thr) <= eps_row[p] and ((jj == 0 and sc[p] == 0.0) or U[p, jj] >= lmax[p] - eps)
            if jj != best and d == 0.0:
                fail("exact tie resolved to the higher index: " + where)
                idx_state[p] = 2
            elif (jj == best) or (0.0 < d <= eps) or on_thr:
                if jj != best or on_thr or abs(U[p, jj] - thr) <= eps:
                    excused += 1
                    idx_state[p] = 1
                else:
                    fail("score zeroed / kept against the threshold: " + where)
                    idx_state[p] = 2
            else:
                fail("index: " + where)
                idx_state[p] = 2
        # mask_all
        want = ref["mask"][k]
        diff = np.flatnonzero(mk != want)
        for p in diff:
            if idx_state[p] == 2:
                continue                 # already counted
            cols = {int(j[p]), int(ref["idx"][k][p]), int(p)}
            eb = 2.0 * c * max(mag_row[p], max(mag[:, s].max() for s in cols), 1e-300)
            near = (0.0 < a_m[p] <= eb) or a_t[p] <= eb or any((0.0 < b_m[s] <= eb) or b_t[s] <= eb for s in cols)
            if near:
                if idx_state[p] == 0:
                    excused += 1
            else:
                fail(f"mask: det {b} template {n} patch {p}: ours {mk[p]:.6g} float64 {want[p]:.6g}; ours idx {int(j[p])} float64 idx "
                     f"{int(ref['idx'][k][p])}; row margin {a_m[p]:.3g} / thr {a_t[p]:.3g}; column margins "
                     + ", ".join(f"[{s}] {b_m[s]:.3g} / thr {b_t[s]:.3g}" for s in sorted(cols)) + f"; eps {eb:.3g}")
        # sim_avg: the reduction alone, on the kernel's own records
        terms = sc * mk.astype(np.float64)
        want_avg = terms.sum() / 256.0 if mk.sum() > 0 else 0.0
        got = float(ours["sim_avg"][b, n])
        checked += 1
        if (mk.sum() == 0 and got != 0.0) or abs(got - want_avg) > 256.0 * 2.0 ** -24 * np.abs(terms).sum() / 256.0 + 1e-45:
            fail(f"sim_avg: det {b} template {n}: ours {got:.9g}, float64 sum of ours score * mask / 256 = {want_avg:.12g} "
                 f"({int((mk != 0).sum())} masks set)")
    return dict(checked=checked, excused=excused, failed=failed, max_ratio=max_ratio, first=first)


MATCH_MUTANTS = ("tie_higher", "zero_row_first_live", "colmax_drops_a_row_group", "last_band_transposed", "wrong_direction",
                 "avg_by_count", "score_offset")


def match_mutant(kind, case, ref, thr=0.5, patch_thr=3.0, direction="tar2src"):
    """Subtly wrong matcher results derived from the float64 ones -- each a bug match_tiles_split_kernel could have; the checker must
    reject every one (tests/test_stage_refs.py).  case: match_blocks_case's dict, ref: match_tiles_f64 of it over all tiles."""
    B, N = case["B"], case["N"]
    ours = match_ref_as_ours(ref, B, N)
    if kind == "tie_higher":                   # (a) a planted tie resolved to the higher index
        lo_, hi_ = MATCH_DUP_TMPL
        tm = case["tm"][case["labels"]]                                               # (B, N, 256)
        tied = (ours["idx"] == lo_) & (ours["score"] != 0) & (tm[:, :, lo_] == tm[:, :, hi_])[:, :, None]
        assert tied.any()
        ours["idx"][tied] = hi_
    elif kind == "zero_row_first_live":        # (b) "maximum 0 means index 0" dropped: an all-zero row returns the first live patch
        tm = case["tm"][case["labels"]]
        first_live = np.where((tm != 0).any(-1), (tm != 0).argmax(-1), 0)              # (B, N)
        zero = ours["score"] == 0
        ours["idx"] = np.where(zero, first_live[:, :, None], ours["idx"]).astype(np.uint8)
    elif kind == "colmax_drops_a_row_group":   # (c) the column maxima miss the first row group (compacted rows 0..63), tiles with nrb >= 6
        def drop(qm, sm):
            live = np.flatnonzero(qm != 0)
            d = np.zeros(P, bool)
            if -(-live.size // 32) >= 6:
                d[live[:64]] = True
            return d
        bad = match_tiles_f64(case["q_hi"], case["q_lo"], case["b_hi"], case["b_lo"], case["qm"], case["tm"], case["labels"], thr, patch_thr,
                              direction, _drop=drop)
        ours = match_ref_as_ours(bad, B, N)
    elif kind == "last_band_transposed":       # (d) tile (b, n) of the ragged last band of 8 crops computed as tile (n, b)
        good = match_ref_as_ours(ref, B, N)
        for b in range(8 * ((B - 1) // 8), B):
            for n in range(min(N, B)):
                for k in ours:
                    ours[k][b, n] = good[k][n, b]
    elif kind == "wrong_direction":            # (e) the other search direction
        other = "src2tar" if direction == "tar2src" else "tar2src"
        bad = match_tiles_f64(case["q_hi"], case["q_lo"], case["b_hi"], case["b_lo"], case["qm"], case["tm"], case["labels"], thr, patch_thr, other)
        ours = match_ref_as_ours(bad, B, N)
    elif kind == "avg_by_count":               # (f) sim_avg = the mean over the valid patches instead of sum / 256
        cnt = (ours["mask"] != 0).sum(-1)
        ours["sim_avg"] = np.where(cnt > 0, ours["sim_avg"] * 256.0 / np.maximum(cnt, 1), 0.0).astype(np.float32)
    elif kind == "score_offset":               # (g) scores off by 8e-6
        ours["score"] = np.where(ours["score"] != 0, ours["score"] + np.float32(8e-6), ours["score"]).astype(np.float32)
    else:
        raise ValueError(kind)
    return ours


# name -> (which, C, sim_threshold, patch_threshold, direction, two-plane bank, objects, anti-correlated, more than this many valid
# correspondences): the cases of tests/test_gpu_matcher_f64.py; tests/test_stage_refs.py asserts their preconditions on the CPU
MATCH_CASES = {
    "blocks_a": ("a", 64, 0.5, 3.0, "tar2src", True, 1, False, 600),
    "blocks_b": ("b", 64, 0.5, 3.0, "tar2src", True, 1, False, 600),
    "blocks_a_c1024": ("a", 1024, 0.5, 3.0, "tar2src", True, 1, False, 600),
    "blocks_a_c32": ("a", 32, 0.5, 3.0, "tar2src", True, 1, False, 600),
    "blocks_a_c96": ("a", 96, 0.5, 3.0, "tar2src", True, 1, False, 600),
    "src2tar": ("a", 64, 0.5, 3.0, "src2tar", True, 1, False, 600),
    "no_cycle_check": ("a", 64, 0.5, 0.0, "tar2src", True, 1, False, 600),
    "thr_zero": ("a", 64, 0.0, 3.0, "tar2src", True, 1, False, 600),
    "thr_negative": ("a", 64, -0.25, 3.0, "tar2src", True, 1, True, 100),
    "one_plane_bank": ("a", 64, 0.5, 3.0, "tar2src", False, 1, False, 600),
    "three_objects": ("a", 64, 0.5, 3.0, "tar2src", True, 3, False, 600),
}
_match_cache = {}


def match_case(name):
    """-> (case, ref, c) of MATCH_CASES[name], computed once per process and shared (treat as read-only): the inputs, the float64
    records of every tile and the value coefficient."""
    if name not in _match_cache:
        which, C, thr, pthr, direction, two_plane, O, anti, _ = MATCH_CASES[name]
        case = match_blocks_case(which, C, O=O, labels=MATCH_O3_LABELS if O == 3 else None, anti=anti)
        if not two_plane:
            case["b_lo"] = None
        case.update(thr=thr, patch_thr=pthr, direction=direction)
        ref = match_tiles_f64(case["q_hi"], case["q_lo"], case["b_hi"], case["b_lo"], case["qm"], case["tm"], case["labels"], thr, pthr, direction)
        c = match_value_coeff(case["q_hi"], case["q_lo"], case["b_hi"], case["b_lo"], case["labels"])
        _match_cache[name] = (case, ref, c)
    return _match_cache[name]


# ---------------------------------------------------------------------------------------------------------------- IST convolutions at the ends of the plane range
# (tests/test_gpu_ist_range.py.)  Two plane conventions: "planes" = hi = f16(8 x), lo = f16(8 x - hi), value (hi + lo) / 8, legal while
# |8 x| <= 65504 (gp_conv2d_planes, the default kernels); "wide" = hi = f16(x), lo = f16((x - hi) 2^11), value hi + lo / 2048, legal while
# |x| <= 65504 (gp_conv2d_nhwc_split, the fallback).
F16_MAX = 65504.0
ACT_LIMIT = F16_MAX / 8.0                    # 8188: the largest |x| of the default kernels' planes
WIDE_LO = 2048.0
PLANES_FLOOR = (2.0 ** -22, 2.0 ** -28)      # (relative, absolute) term of a plane OUTPUT (hi + lo) / 8: 22 bits of 8 y; the lo plane's f16 subnormal floor, 2^-25 / 8
WIDE_FLOOR = (2.0 ** -22, 2.0 ** -35)        # hi + lo / 2048: 22 bits; the lo plane's f16 subnormal spacing 2^-24 / 2048

# route -> (Cin, Cout, k, stride, pad, H = W, B): the smallest launches of gp_conv2d_planes that reach each kernel instantiation
# (Cin % 32 = 0, Cout % 64 = 0, B OH OW % 256 = 0; gp_plan256.h: gp_conv256_plan, launched by gp_conv256.hip's gp_conv2d_planes)
CONV_GUARD_ROUTES = {
    "gather_ni2": (32, 128, 3, 2, 1, 32, 1),
    "gather_ni3_1x1": (32, 192, 1, 2, 0, 32, 1),
    "gather_ni4_two_channel_tiles": (32, 512, 3, 2, 1, 32, 1),
    "gather_3x3_s1_not_16": (32, 128, 3, 1, 1, 8, 4),
    "gather_cut_tiles": (256, 512, 3, 2, 1, 32, 4),
    "halo_cout64": (32, 64, 3, 1, 1, 16, 1),
    "halo_ni2_serial": (64, 128, 3, 1, 1, 16, 1),
    "halo_ni2_parallel": (64, 128, 3, 1, 1, 16, 8),
    "halo_ni3_parallel": (64, 192, 3, 1, 1, 16, 8),
    "halo_ni4_parallel": (64, 256, 3, 1, 1, 16, 8),
}
RES_PLANT_BETA = 150.0                       # see conv_guard_residual_case


def conv_out_size(hw, k, stride, pad):
    return (hw + 2 * pad - k) // stride + 1


def split_wide_host(x):
    """The two-accumulator convention on the host: hi = f16(x), lo = f16((x - hi) * 2048), one IEEE operation per step."""
    x = torch.as_tensor(x, dtype=torch.float32)
    hi = x.to(torch.float16)
    lo = ((x - hi.to(torch.float32)) * torch.tensor(WIDE_LO, dtype=torch.float32)).to(torch.float16)
    return hi, lo


def wide_value(hi, lo):
    return hi.double() + lo.double() / WIDE_LO


def _guard_base(route, seed):
    cin, cout, k, stride, pad, hw, B = CONV_GUARD_ROUTES[route]
    rs = np.random.RandomState(seed + cin + cout + 7 * k + hw + B)
    X = rs.standard_normal((B, hw, hw, cin)).astype(np.float32)
    Wt = (rs.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    oh = conv_out_size(hw, k, stride, pad)
    return rs, dict(X=X, Wt=Wt, R=None, stride=stride, pad=pad, oh=oh, npix=B * oh * oh, cout=cout, route=route)


def conv_guard_zero_channel_case(route, v, seed=0):
    """Small random inputs and weights, alpha = 1, and ONE output channel `co` (the third from the end: inside the last 4-channel quad
    of the last channel tile) whose weights are all zero and whose beta is v: that channel's epilogue value is 0 * 1 + v = v exactly
    at every pixel, 8 v exactly in f32."""
    rs, case = _guard_base(route, seed)
    cout = case["cout"]
    co = cout - 3
    case["Wt"][co] = 0.0
    beta = rs.standard_normal(cout).astype(np.float32)
    beta[co] = v
    case.update(alpha=np.ones(cout, np.float32), beta=beta, co=co, v=float(v))
    return case


def conv_guard_residual_case(route, where, over, seed=1):
    """Small random inputs, weights, BatchNorm and residual; ONE output is pushed to about 8300 (over = True: above the limit 8188 by
    more than 1 %) or about 8000 (clean twin: below it by more than 1 %) through the residual: where = "first" -> pixel 0 / channel 0 (the
    first row and column of the first tile), "last" -> the last pixel / last valid channel of the last tile.
    A residual of 8300 itself cannot be written into the x 8 planes (66400 > 65504: the residual's own hi plane would hold inf), so the
    planted element carries 8150 / 7850 and beta of that channel the other RES_PLANT_BETA = 150: the float64 OUTPUT is 8300 / 8000 plus
    the convolution's few units, every operand is a legal plane value."""
    rs, case = _guard_base(route, seed)
    cout, npix, oh = case["cout"], case["npix"], case["oh"]
    alpha = rs.uniform(0.5, 1.5, cout).astype(np.float32)
    beta = rs.standard_normal(cout).astype(np.float32)
    R = rs.standard_normal((npix, cout)).astype(np.float32)
    pix, co = (0, 0) if where == "first" else (npix - 1, cout - 1)
    beta[co] = RES_PLANT_BETA
    R[pix, co] = (8300.0 if over else 8000.0) - RES_PLANT_BETA
    case.update(alpha=alpha, beta=beta, R=R.reshape(-1, oh, oh, cout), pix=pix, co=co, over=bool(over))
    return case


def conv_range_case(cin, cout, k, stride, pad, hw, B, seed, top=3.5, limit=ACT_LIMIT, res=True):
    """Convolution + BatchNorm + residual + ReLU far from unit scale.  NHWC inputs and a residual of per-pixel scale 10^U(-4, top) times
    U(-1, 1) (top = 3.5: values from 1e-4 to about 3000), weights N(0, 1) / sqrt(K), alpha in [0.5, 1.5], beta N(0, 1) x the median
    pixel scale; the special values of split_values_case (exact f16 values, ties of the hi rounding, lo-plane subnormals) planted into
    the channels of one input pixel and -- those up to 4096 -- of one residual pixel.  Inputs, beta and residual (not the planted values)
    are then multiplied by ONE factor (0.3 .. 3) so that the float64 output peaks near 0.8 of `limit` (ReLU is homogeneous: the output
    scales with them); tests/test_stage_refs.py asserts the peak of |y| between 0.5 and 0.95 of it on the values the planes hold."""
    rs = np.random.RandomState(seed)
    oh = conv_out_size(hw, k, stride, pad)
    K = cin * k * k
    sx = 10.0 ** rs.uniform(-4.0, top, (B, hw, hw, 1))
    X = rs.uniform(-1.0, 1.0, (B, hw, hw, cin)) * sx
    Wt = (rs.standard_normal((cout, cin, k, k)) / np.sqrt(K)).astype(np.float32)
    alpha = rs.uniform(0.5, 1.5, cout).astype(np.float32)
    beta = rs.standard_normal(cout) * np.median(sx)
    R = rs.uniform(-1.0, 1.0, (B, oh, oh, cout)) * 10.0 ** rs.uniform(-4.0, top, (B, oh, oh, 1)) if res else None
    special = split_values_case(40, seed)[1:23].astype(np.float64)
    n = min(len(special), cin)
    px = (B - 1, hw // 2, hw // 3)
    pr = (0, oh // 3, oh // 2)
    rspecial = special[np.abs(special) <= 4096.0][:cout]

    def peak(s):
        x, r = X * s, (None if R is None else R * s)
        x[px][:n] = special[:n]
        if r is not None:
            r[pr][:len(rspecial)] = rspecial
        x, b, r = x.astype(np.float32), (beta * s).astype(np.float32), (None if r is None else r.astype(np.float32))
        y = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(Wt).double(), stride=stride, padding=pad)
        y = y * torch.from_numpy(alpha).double()[None, :, None, None] + torch.from_numpy(b).double()[None, :, None, None]
        if r is not None:
            y = y + torch.from_numpy(r).double().permute(0, 3, 1, 2)
        return float(torch.relu(y).max()), x, b, r

    s = 1.0
    for _ in range(3):          # the planted values do not scale: a second and third pass settle the factor
        p, x, b, r = peak(s)
        s *= 0.8 * limit / p
    p, x, b, r = peak(s)
    return dict(X=x, Wt=Wt, alpha=alpha, beta=b, R=r, stride=stride, pad=pad, oh=oh, npix=B * oh * oh, cout=cout, factor=s, limit=limit,
                planted_x=px, planted_r=pr, n_special=n)


def conv_case_values(case, wide=False):
    """The float64 values the kernel reads: the host split of the case's f32 arrays (bit for bit the planes gp_split_planes /
    split_planes make on the device; the GPU tests pass the device's planes instead) -> (x, w, r) float64 tensors, x / r NHWC."""
    if wide:
        val = lambda t, _s: wide_value(*split_wide_host(t))                                  # noqa: E731
    else:
        val = lambda t, s: planes_value(*split_planes_host(t, s), s)                          # noqa: E731
    return val(case["X"], 8.0), val(case["Wt"], 64.0), None if case["R"] is None else val(case["R"], 8.0)


def conv_range_reference(x, w, alpha, beta, r, stride, pad, relu=True):
    """float64 reference and per-output bound coefficient of conv + BN + residual + ReLU on the values given (x (B, H, W, Cin), w (Cout,
    Cin, k, k), r (B, OH, OW, Cout) or None: float64, what the planes hold) -> dict of (B, Cout, OH, OW) float64 tensors
      y    the float64 result,
      mag  conv(|x|, |w|) |alpha| + |beta| + |r|, the magnitude every rounding error of an evaluation scales with,
      y32  torch's own float32 evaluation of the same expression (operands converted exactly: plane values fit 24 bits),
    and c = 2 x max |y32 - y| / mag (match_value_coeff's method; the factor 2 covers another summation order).  Nothing here comes from
    the kernel under test."""
    F = torch.nn.functional
    a, b = torch.as_tensor(alpha).double()[None, :, None, None], torch.as_tensor(beta).double()[None, :, None, None]
    xc, rc = x.permute(0, 3, 1, 2), (None if r is None else r.permute(0, 3, 1, 2))
    y = F.conv2d(xc, w, stride=stride, padding=pad) * a + b
    mag = F.conv2d(xc.abs(), w.abs(), stride=stride, padding=pad) * a.abs() + b.abs()
    y32 = F.conv2d(xc.float(), w.float(), stride=stride, padding=pad) * a.float() + b.float()
    if rc is not None:
        y, mag, y32 = y + rc, mag + rc.abs(), y32 + rc.float()
    if relu:
        y, y32 = torch.relu(y), torch.relu(y32)
    ratio = (y32.double() - y).abs() / mag.clamp_min(1e-300)
    ok = torch.isfinite(ratio)
    return dict(y=y, mag=mag, y32=y32.double(), c=2.0 * float(ratio[ok].max()))


def conv_bound(ref, floor=None):
    """c mag + floor per output; floor = (relative, absolute) of the output's plane format, None for the f32 output."""
    bound = ref["c"] * ref["mag"]
    if floor is not None:
        bound = bound + floor[0] * ref["y"].abs() + floor[1]
    return bound


def conv_bound_worst(got, ref, floor=None, where=None):
    """-> (worst err / bound, its index) over the outputs selected by `where` (default: all).  A non-finite `got` counts as inf."""
    err = (got - ref["y"]).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    q = err / conv_bound(ref, floor)
    if where is not None:
        q = torch.where(where, q, torch.zeros_like(q))
    i = int(q.argmax())
    return float(q.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, q.shape))


CONV_MUTANTS = ("lo_planes_dropped", "residual_hi_only", "small_outputs_flushed")


def conv_mutant(kind, case, wide=False):
    """Three subtly wrong results, derived from float64 (no other error): the activations' lo planes dropped, the residual added as its
    hi plane only, outputs below 2^-10 max |y| flushed to zero.  (B, Cout, OH, OW) float64."""
    x, w, r = conv_case_values(case, wide)
    if kind == "lo_planes_dropped":
        hi = split_wide_host(case["X"])[0].double() if wide else split_planes_host(case["X"], 8.0)[0].double() / 8.0
        return conv_range_reference(hi, w, case["alpha"], case["beta"], r, case["stride"], case["pad"])["y"]
    if kind == "residual_hi_only":
        hi = split_wide_host(case["R"])[0].double() if wide else split_planes_host(case["R"], 8.0)[0].double() / 8.0
        return conv_range_reference(x, w, case["alpha"], case["beta"], hi, case["stride"], case["pad"])["y"]
    if kind == "small_outputs_flushed":
        y = conv_range_reference(x, w, case["alpha"], case["beta"], r, case["stride"], case["pad"])["y"]
        return torch.where(y.abs() < 2.0 ** -10 * y.abs().max(), torch.zeros_like(y), y)
    raise ValueError(kind)


# part B's runs: name -> (route or shape, top exponent, wide); shapes (Cin, Cout, k, stride, pad, H = W, B)
CONV_RANGE_CASES = {
    "gather_ni2": (CONV_GUARD_ROUTES["gather_ni2"], 3.5, False),
    "gather_ni3_1x1": (CONV_GUARD_ROUTES["gather_ni3_1x1"], 3.5, False),
    "halo_ni2_serial": (CONV_GUARD_ROUTES["halo_ni2_serial"], 3.5, False),
    "halo_ni4_parallel": (CONV_GUARD_ROUTES["halo_ni4_parallel"], 3.5, False),
    "wide_3x3_s1": ((32, 64, 3, 1, 1, 16, 2), 4.4, True),
    "wide_1x1_s2": ((64, 192, 1, 2, 0, 16, 2), 4.4, True),
}
_conv_range_cache = {}


def conv_range_named(name):
    """-> the case of CONV_RANGE_CASES[name], built once per process (treat as read-only)."""
    if name not in _conv_range_cache:
        shape, top, wide = CONV_RANGE_CASES[name]
        _conv_range_cache[name] = conv_range_case(*shape, seed=1000 + len(name) + shape[1], top=top, limit=F16_MAX if wide else ACT_LIMIT)
    return _conv_range_cache[name]


def resize_guard_image(over, IH=24, IW=40, seed=5):
    """(2, 3, IH, IW) f32 noise whose first pixel of crop 1 / channel 2 is 8300 (over) or 8100: align_corners maps a corner onto itself
    (source coordinate 0, interpolation weights exactly 1 and 0), so the bilinear resize peaks at exactly that value in any precision."""
    x = torch.randn(2, 3, IH, IW, generator=torch.Generator().manual_seed(seed))
    x[1, 2, 0, 0] = 8300.0 if over else 8100.0
    return x


# ---------------------------------------------------------------------------------------------------------------- the IST ResNet, layer by layer
def resnet_layer_maxima(backbone, x):
    """The float64 / float32 torch forward of oracle/ist_torch.py (whatever dtype `backbone` and `x` hold) with the largest |value| of every
    tensor on the way -> (rec, written, features):
      rec      {name: max |.|} of the resized input, every Conv2d and BatchNorm2d output (forward hooks), the stem's and every block's output;
      written  the subset the split path stores as f16 PLANES -- the resized input, relu(bn1(.)) of the stem and of every block (the maximum
               of the positive part: ReLU runs before the store), the downsample shortcut's BatchNorm output, every block's output.  Convolution
               outputs before BatchNorm and bn2 before the residual live in f32 accumulators only; the head's output is f32;
      features the (b, D, 16, 16) output."""
    from oracle import ist_torch

    F = torch.nn.functional
    rec, written, hooks = {}, {}, []

    def hook(name):
        def fn(_mod, _inp, out):
            rec[name] = max(rec.get(name, 0.0), float(out.abs().max()))
            if name.endswith("bn1"):
                written["relu(" + name + ")"] = max(written.get("relu(" + name + ")", 0.0), float(out.max()))
            elif name.endswith("downsample.1"):
                written[name] = rec[name]
        return fn

    for name, m in backbone.named_modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d)):
            hooks.append(m.register_forward_hook(hook(name)))
    try:
        with torch.no_grad():
            y = F.interpolate(x, (backbone.input_size, backbone.input_size), mode="bilinear", align_corners=True)
            rec["resize"] = written["resize"] = float(y.abs().max())
            y = F.relu(backbone.bn1(backbone.conv1(y)))
            for li, stage in enumerate((backbone.layer1, backbone.layer2, backbone.layer3, backbone.layer4), 1):
                for bi, blk in enumerate(stage):
                    y = ist_torch.basic_block(blk, y)
                    rec[f"layer{li}.{bi}.out"] = written[f"layer{li}.{bi}.out"] = float(y.abs().max())
            feats = backbone.layer4_outconv(y)
    finally:
        for h in hooks:
            h.remove()
    return rec, written, feats


def maxima_line(d):
    return ", ".join(f"{n} {v:.4g}" for n, v in d.items())
