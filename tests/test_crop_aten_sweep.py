"""CPU: the numpy restatement of the crop stage (oracle/crop_numpy.py) against ATen itself -- the reference's op chain run
with torch ops (gigapose_testing/crop_aten.py) -- over every box family: all long sides 1..700, every doubled / kept
extent, the identity and 2x scales, clamped boxes and the refused ones; targets 224, 112 and 37 on frames of 97x131 and
300x420, on a one-channel index image (pixel = 1 + y*W + x, exact in float32: a wrong source pixel is a wrong value).

Images bit for bit; M[0,0], M[1,1] and the constant entries bit for bit against torch.matmul of the two matrices, the
translations to 1 ulp (matmul order); both sides refuse the same boxes; outside the refused family ATen refuses none.

Two defects this sweep found in the restatement (and, the same arithmetic, in gp_crop_geom.h), with the number of cases
that differed in at least one pixel before the fix, of the cases in this file:
  scale class    `target / int32_tensor` is reciprocal() * target in torch, two float32 roundings, not the correctly
                 rounded quotient: another scaled size, another pad, for about one long side in five;
  kernel class   ATen's CPU kernel with the `dst` / `dst >> 1` shortcuts runs only when out_h + out_w <= 128; the generic
                 kernel floors dst * (float)(1 / scale) also for a doubled or kept extent.
The counts are recorded in DESIGN.md ("Crop geometry held to ATen")."""
import numpy as np
import pytest
import torch

from gigapose_testing import crop_aten
from oracle import crop_numpy

FRAMES = [(97, 131), (300, 420)]
TARGETS = [224, 112, 37]
CASES = [(H, W, T) for (H, W) in FRAMES for T in TARGETS]


def _families(H, W, T):
    return crop_aten.families(H, W, T, seed=1000 + H + T, thin=(T != 224))   # long sides thinned by target, nothing else


def sweep(crop_fn, H, W, T):
    """Every family at one frame and target: (number of cases, list of (family, box, what differed))."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                 # thousands of tiny ops: a thread pool only costs (no kernel is chosen by it)
    try:
        return _sweep(crop_fn, H, W, T)
    finally:
        torch.set_num_threads(threads)


def _sweep(crop_fn, H, W, T):
    img_np = crop_aten.index_image(H, W)
    img_t = torch.from_numpy(img_np)
    bad, n = [], 0
    for name, boxes in _families(H, W, T).items():
        assert len(boxes) > 0, name
        for box in boxes:
            n += 1
            ref, ref_M, err = crop_aten.aten_crop_or_error(img_t, box, T)
            if name != "refused":
                assert err is None, f"{name} {box} at {T}: ATen refused a box outside the refused family: {err}"
            else:
                assert err is not None, f"refused family: ATen accepted {box} at {T}"
            try:
                out, M = crop_fn(img_np[None], np.asarray([box], np.int64), T)
            except ValueError:
                if err is None:
                    bad.append((name, box, "refused by the restatement alone"))
                continue
            if err is not None:
                bad.append((name, box, "refused by ATen alone"))
                continue
            if not np.array_equal(out[0].view(np.uint32), ref.view(np.uint32)):
                bad.append((name, box, "pixels"))
            try:
                crop_aten.assert_M(M[0], ref_M)
            except AssertionError:
                bad.append((name, box, "M"))
    return n, bad


def classify(bad, H, W, T):
    """Distinct mismatching boxes by defect class (a box can be in both).  `scale_same_size`: of those in neither
    class by size, the boxes whose two scales differ all the same -- same scaled size, another source map."""
    px = {b for (_, b, what) in bad if what == "pixels"}
    other = [b for b in px if not crop_aten.is_scale_class(b, H, W, T) and not crop_aten.is_generic_kernel_class(b, H, W, T)]
    return dict(pixels=len(px), scale=sum(crop_aten.is_scale_class(b, H, W, T) for b in px),
                kernel=sum(crop_aten.is_generic_kernel_class(b, H, W, T) for b in px),
                scale_same_size=sum(crop_aten.recip_scale(max(b[2] - b[0], b[3] - b[1]), T)
                                    != crop_aten.div_scale(max(b[2] - b[0], b[3] - b[1]), T) for b in other), neither=len(other),
                M=len({b for (_, b, what) in bad if what == "M"}), refusal=sum("refused" in what for (_, _, what) in bad))


@pytest.mark.parametrize("H,W,T", CASES)
def test_restatement_equals_aten_on_every_family(H, W, T):
    n, bad = sweep(crop_numpy.crop_resize_pad, H, W, T)
    assert n > 1000
    assert not bad, f"{len(bad)} of {n} cases differ from ATen {classify(bad, H, W, T)}; first: {bad[:5]}"


@pytest.mark.parametrize("H,W,T", CASES)
def test_families_carry_both_defect_classes(H, W, T):
    """Pure size arithmetic: a generator change must not leave the sweep without the cases it was written for."""
    fam = _families(H, W, T)
    live = [b for k, v in fam.items() if k != "refused" for b in v]
    assert all(crop_aten.scaled_nonempty(b, H, W, T) for b in live)
    assert not any(crop_aten.scaled_nonempty(b, H, W, T) and b[0] >= 0 and b[0] < W and b[1] < H for b in fam["refused"])
    n_scale = sum(crop_aten.is_scale_class(b, H, W, T) for b in live)
    n_scale_nonsquare = sum(crop_aten.is_scale_class(b, H, W, T) and b[2] - b[0] != b[3] - b[1] for b in live)
    assert n_scale_nonsquare >= 50, (n_scale, n_scale_nonsquare)
    n_wide = sum(crop_aten.is_width_only_doubled(b, H, W, T) for b in live)
    n_tall = sum(crop_aten.is_width_only_doubled((b[1], b[0], b[3], b[2]), W, H, T) for b in live)
    cw_ch = [crop_aten.first_resize(b, H, W, T) for b in live]
    n_both = sum(w1 == 2 * cw and h1 == 2 * ch for cw, ch, w1, h1, _ in cw_ch)
    assert n_wide >= 10 and n_tall >= 10 and n_both >= 10, (n_wide, n_tall, n_both)
    # the measured trigger: the generic kernel (out_h + out_w > 128) with a doubled / kept extent.  A target of 37 or
    # less never reaches it (out_h + out_w <= 2T): there the sweep holds that the shortcuts DO apply.
    n_kernel = sum(crop_aten.is_generic_kernel_class(b, H, W, T) for b in live)
    sums = {w1 + h1 for _, _, w1, h1, _ in cw_ch}
    if 2 * T > crop_aten.VECTORIZED_MAX_HW:
        assert n_kernel >= 10, n_kernel
        assert {128, 129} <= sums                 # both sides of ATen's kernel selection
    else:
        assert n_kernel == 0


def test_scale_model_is_torchs_rtruediv():
    """float32(1) / float32(n) * float32(T) is `T / int32_tensor` bit for bit, and differs from the rounded quotient."""
    n = np.arange(1, 4097)
    differ = 0
    for T in TARGETS:
        ref = (T / torch.arange(1, 4097, dtype=torch.int32)).numpy()
        model = (np.float32(1.0) / n.astype(np.float32)) * np.float32(T)
        np.testing.assert_array_equal(model.view(np.uint32), ref.view(np.uint32))
        assert [crop_aten.recip_scale(int(k), T) for k in (1, 23, 700)] == [float(ref[0]), float(ref[22]), float(ref[699])]
        differ += int((model != np.float32(T) / n.astype(np.float32)).sum())
    assert differ > 1000
