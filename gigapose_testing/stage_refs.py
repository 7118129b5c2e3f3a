"""Input builders and float64 references of the stage tests of the split path's non-GEMM kernels (tests/test_gpu_layernorm_planes.py,
test_gpu_ist_split.py, test_gpu_stem_planes.py, test_gpu_plane_producers.py).  numpy / torch on the CPU only: nothing here touches a GPU or
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
    raise ValueError(kind)


def attention_bound(e32, scale):
    """The kernel's bound on max |err| / max |ref|: twice torch's own f32 evaluation of the formula on the same values (a different
    summation order and nothing else), not below the stage bound the kernel already had (2e-6 on x 8 planes, 4e-6 on others), plus the
    output planes' 22 bits."""
    return max(2.0 * e32, 2e-6 if scale == 8.0 else 4e-6) + 2.0 ** -21
