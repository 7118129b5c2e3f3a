"""GPU: attention_split_kernel (gp_vit.hip; stage entry gp_attention_split_scaled) on the PRODUCT library against float64 softmax
attention, on inputs that drive each of its paths to an edge -- the two stage tests it had (test_gpu_split.py, test_gpu_plane_scales.py)
use ViT-S geometry and Gaussian q / k with a logit spread of 2, which exercises none of:
  * the running reference mb = max(m_run, cmax - 15) across the three chunks of 96 keys, and the alpha rescale (descending / ascending);
  * P = 2^15 p as two f16 halves with flushed subnormals (peaked, sink: weights from 1 down to nothing in one row);
  * keys 257..287 masked in the last tile only, whose one valid key is key 256 (sink256, sink);
  * query 256 on its own vector-ALU path, where wave 0 adds key 256 (every class reports that row alone too);
  * the single f32 rounding of the scaled logit (offset: logits near 300);
  * exact 1 / 257 weights (uniform, zero_q: the output is the column mean of V).
Classes, their constructions and the preconditions that keep them what they are named after: gigapose_testing/stage_refs.py
(attention_case, attention_preconditions); tests/test_stage_refs.py shows without a GPU that the reference rejects a kernel that drops
key 256, scales by 1 / sqrt(63) or takes the chunks relative to their own maxima.  Geometries: ViT-L (3 crops x 16 heads) and ViT-B (5 x 12:
B H is not a multiple of the XCD chunk, Mpad = 1536 leaves 251 pad rows).

Bound (stage_refs.attention_bound): max |err| / max |ref| <= max(2 e32, floor) + 2^-21, e32 = the error of torch's own f32 evaluation of
softmax(q k^T / 8) v on the CPU on the same plane values, floor = the stage bound the kernel already had (2e-6 on x 8 planes, 4e-6 on
others).  Arithmetic restated: HF modeling_dinov2.py:207-229."""
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from test_gpu_split import planes8

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL_HI, SENTINEL_LO = 1234.0, -0.40625      # exact f16 values no output of these cases equals in a whole row

CASES = [(cls, scale) for cls in sr.ATTN_CLASSES for scale in ((8.0, 0.5) if cls in sr.ATTN_OTHER_SCALE else (8.0,))]


def launch(hi, lo, B, H, Mpad, scale):
    ohi = torch.full((Mpad, 64 * H), SENTINEL_HI, dtype=torch.float16, device=DEV)
    olo = torch.full((Mpad, 64 * H), SENTINEL_LO, dtype=torch.float16, device=DEV)
    _lib.call("gp_attention_split_scaled", _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(ohi), _lib.ptr(olo), _lib.i(B), _lib.i(H), _lib.i(64 * H), _lib.i(Mpad),
              _lib.f(scale), _lib.stream_ptr())
    torch.cuda.synchronize()
    return ohi, olo


@pytest.mark.parametrize("cls,scale", CASES)
@pytest.mark.parametrize("B,H", [(3, 16), (5, 12)])
def test_attention_split_vs_float64_on_adversarial_inputs(B, H, cls, scale):
    M = B * sr.T_TOK
    Mpad = (M + 255) // 256 * 256
    qkv = torch.full((Mpad, 3 * 64 * H), 1000.0)                    # pad rows: finite values the kernel has no business reading
    qkv[:M] = sr.attention_case(cls, B, H, seed=5)
    assert float(qkv[:M].abs().max()) * scale < 8190.0
    hi, lo = planes8(qkv.to(DEV), scale)                            # gp_split_planes: pinned bit for bit by test_gpu_plane_producers.py
    vals = sr.planes_value(hi[:M].cpu(), lo[:M].cpu(), scale)       # what the kernel is given, in float64
    pre = sr.attention_preconditions(cls, sr.attention_logits(vals, B, H))
    assert pre and all(ok for _, ok in pre.values()), f"class {cls} is no longer what it is named after: {pre}"
    ref = sr.attention_ref(vals, B, H)
    rmax = float(ref.abs().max())
    e32 = float((sr.attention_ref(vals, B, H, torch.float32).double() - ref).abs().max()) / rmax
    bound = sr.attention_bound(e32, scale)
    if cls in ("uniform", "zero_q"):
        mean = sr.attention_qkv(vals, B, H)[2].mean(dim=2, keepdim=True).expand(-1, -1, sr.T_TOK, -1).permute(0, 2, 1, 3)
        assert float((ref - mean).abs().max()) < 1e-14

    _lib.status_word(DEV).zero_()
    ohi, olo = launch(hi, lo, B, H, Mpad, scale)
    _lib.check_status()
    got = sr.planes_value(ohi[:M].cpu(), olo[:M].cpu(), scale).view(B, sr.T_TOK, H, 64)
    err = float((got - ref).abs().max()) / rmax
    err256 = float((got[:, 256] - ref[:, 256]).abs().max()) / rmax
    print(f"attention split {cls:10s} B={B} H={H} scale {scale:g}: kernel {err:.3e}  f32 CPU reference {e32:.3e}  ratio {err / e32:.2f}  "
          f"bound {bound:.3e}  query 256 alone {err256:.3e}")
    assert torch.isfinite(got).all()
    assert err <= bound, f"{err:.3e} > {bound:.3e} ({err / e32:.2f} x the f32 reference's error)"
    assert err256 <= bound, f"query 256: {err256:.3e} > {bound:.3e}"
    assert sr.planes_well_formed(ohi[:M].cpu(), olo[:M].cpu())
    # rows >= B * 257 are nobody's: still the sentinel
    assert bool((ohi[M:] == SENTINEL_HI).all()) and bool((olo[M:] == SENTINEL_LO).all()), "pad rows of the output planes were written"
    # a second launch is bit-equal to the first
    ohi2, olo2 = launch(hi, lo, B, H, Mpad, scale)
    assert torch.equal(ohi2, ohi) and torch.equal(olo2, olo), "attention_split_kernel is not deterministic"
