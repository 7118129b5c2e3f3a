"""GPU: the ViT embedding as the patch-embed GEMM's epilogue (gp_gemm.hip: GP_EPI_EMBED -- + bias, + position table, column
b * 256 + p re-indexed to token b * 257 + 1 + p of the residual stream, class-token columns, zeroed pad columns) against a float64
restatement of HF modeling_dinov2.py:97-112 (and :199-380 for the one-block case).

The GEMM-then-embed_kernel pair this replaces computed (acc + bias) + pos in the same order, so the values are the parent's bit for
bit; each bound below is the parent commit's own max |error| against the same restatement on the same seeded inputs, measured once on
an MI355X (the figure is next to it).  tests/test_gpu_vit_f32_stages.py holds the embedding bit-equal to the oracle's chain GEMM in
chain numerics, pad columns included; here the product's default numerics run, at both widths that matter."""
import pytest
import torch

from gigapose_amd import _lib
from gigapose_amd.vit import Dinov2ViT
from gigapose_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"

# max |x_prenorm - float64| of the parent commit, stop_after_layers = 0 (the embedding alone): (dim, B) -> figure
# (measured 6.958e-06, 8.841e-06, 5.846e-06, 6.949e-06; this commit measures the same figures to the last digit)
PARENT_EMBED_ERR = {(384, 1): 6.96e-06, (384, 3): 8.85e-06, (1024, 1): 5.85e-06, (1024, 3): 6.95e-06}
# the same after one block at ViT-S width, B = 3 (split numerics, the default): measured 1.0303e-05; a forward whose class token
# is zero moves the float64 patch tokens by 1.29
PARENT_ONE_BLOCK_ERR = 1.031e-05


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def make_vit(dim, depth, seed):
    return syn.fill_state_dict(Dinov2ViT(dim, depth, dim // 64), seed).eval().to(DEV).set_numerics("split")


def images(seed, B):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def restated(vit, x, layers, cls_token=None):
    """float64 x_prenorm (B, 257, C) after `layers` blocks."""
    sd = {k: v.detach().double().cpu() for k, v in vit.state_dict().items()}
    B, C, H = x.shape[0], vit.dim, vit.heads
    patches = x.double().reshape(B, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(B, 256, 588)
    t = patches @ sd["patch_embed.proj.weight"].reshape(C, 588).T + sd["patch_embed.proj.bias"]
    cls = sd["cls_token"] if cls_token is None else cls_token
    t = torch.cat([cls.expand(B, 1, C), t], 1) + sd["pos_embed"]
    F = torch.nn.functional
    for i in range(layers):
        p = f"blocks.{i}."
        h = F.layer_norm(t, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        qkv = h @ sd[p + "attn.qkv.weight"].T + sd[p + "attn.qkv.bias"]
        q, k, v = [u.reshape(B, 257, H, 64).transpose(1, 2) for u in qkv.split(C, -1)]
        a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
        o = (a @ v).transpose(1, 2).reshape(B, 257, C)
        t = t + sd[p + "ls1.gamma"] * (o @ sd[p + "attn.proj.weight"].T + sd[p + "attn.proj.bias"])
        h = F.layer_norm(t, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
        m = F.gelu(h @ sd[p + "mlp.fc1.weight"].T + sd[p + "mlp.fc1.bias"])
        t = t + sd[p + "ls2.gamma"] * (m @ sd[p + "mlp.fc2.weight"].T + sd[p + "mlp.fc2.bias"])
    return t


def patch_tokens(vit, x, layers):
    """the forward's patch tokens (B, 256, C) on the CPU, in float64"""
    out = vit.patch_features(x.to(DEV), normalize=False, stop_after_layers=layers)
    torch.cuda.synchronize()
    _lib.check_status()
    return out.reshape(x.shape[0], vit.dim, 256).transpose(1, 2).double().cpu()


def embed_error(dim, B):
    vit = make_vit(dim, 1, 61)
    x = images(62 + B, B)
    ref = restated(vit, x, 0)
    got = patch_tokens(vit, x, 0)
    # the class-token and pad columns are not part of patch_features' result: read them in the workspace (include/gigapose_hip.h)
    mpad = (B * 257 + 255) // 256 * 256
    X = vit._ws[: dim * mpad].view(dim, mpad).double().cpu()
    cls = X[:, : B * 257].reshape(dim, B, 257)[:, :, 0].t()
    return (got - ref[:, 1:]).abs().max().item(), (cls - ref[:, 0]).abs().max().item(), X[:, B * 257:]


def one_block_error():
    vit = make_vit(384, 1, 71)
    x = images(72, 3)
    ref = restated(vit, x, 1)
    got = patch_tokens(vit, x, 1)
    # what the check sees of a wrong class-token column: the patch tokens of a forward whose class token is zero
    moved = (restated(vit, x, 1, cls_token=torch.zeros(1, 1, 384, dtype=torch.float64)) - ref)[:, 1:].abs().max().item()
    return (got - ref[:, 1:]).abs().max().item(), moved


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dim", [384, 1024])
def test_embedding_vs_float64(dim, B):
    err, err_cls, pad = embed_error(dim, B)
    print(f"embedding dim={dim} B={B}: max |patch tokens - float64| {err:.3e} (parent {PARENT_EMBED_ERR[(dim, B)]:.3e}), class tokens {err_cls:.3e}")
    assert err <= PARENT_EMBED_ERR[(dim, B)]
    assert err_cls <= 2.0 ** -24 * 4.0      # one f32 rounding of cls + pos[0] (|.| < 4), made on the host
    assert pad.numel() > 0 and not bool(pad.ne(0).any()), "pad columns of the residual stream must be zero"


def test_one_block_sees_the_class_token_column():
    err, moved = one_block_error()
    print(f"one block, ViT-S width, B=3: max |patch tokens - float64| {err:.3e} (parent {PARENT_ONE_BLOCK_ERR:.3e}); "
          f"a zero class token moves them by {moved:.3e}")
    assert err <= PARENT_ONE_BLOCK_ERR
    assert moved > 100 * PARENT_ONE_BLOCK_ERR   # the bound separates a wrong class-token column from a right one
