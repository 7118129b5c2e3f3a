"""The flow DepthRefiner, HypothesisVerifier and MaskRefiner share -- grouping by object and camera, chunking, scattering the
results back -- through the public classes alone: whatever company an estimate is submitted in, and however the call is chunked,
it gets the bits it gets when it is submitted alone.  Every sum is an integer, so this is exact."""
import numpy as np
import pytest

from gigapose_testing import meshes
from gigapose_testing import refine_cases as rc
from gigapose_testing import verify_cases as vc

pytestmark = pytest.mark.gpu


def scene():
    """Twelve estimates on the small frame: two objects interleaved, two frames with different cam_K, and masks of three kinds --
    one dictionary shared by the hypotheses of a detection, a dictionary of an estimate's own, None."""
    v, f = rc.mesh("boxes")
    sv, sf, _ = meshes.icosphere(1, 45.0)
    models = {1: dict(vertices=v, faces=f, diameter=vc.SCALE), 2: dict(vertices=sv, faces=sf, diameter=90.0)}
    K2 = rc.K * np.asarray([1.25, 1, 1, 1, 1.25, 1, 1, 1, 1]) + np.asarray([0, 0, 3.0, 0, 0, -2.0, 0, 0, 0])
    cameras = {(1, 0): dict(cam_K=rc.K, depth=vc.truth(0)["depth"]), (1, 1): dict(cam_K=K2, depth=vc.truth(1)["depth"])}
    poses = np.concatenate([vc.hypotheses(0), vc.hypotheses(1)])
    est = [dict(scene_id=1, im_id=i // 6 if i % 5 else 1 - i // 6, obj_id=2 if i % 3 == 1 else 1, score=0.9 - 0.01 * i, R=p[:3, :3].copy(), t=p[:3, 3].copy())
           for i, p in enumerate(poses)]
    shared = [vc.segmentation(vc.truth(i)["runs"]) for i in range(2)]
    masks = [None if i % 4 == 2 else shared[i // 6] if i % 3 else dict(shared[i // 6]) for i in range(12)]
    assert len({(e["obj_id"], e["im_id"]) for e in est}) == 4 and sum(m is None for m in masks) == 3 and sum(m is shared[0] for m in masks) >= 2
    return models, cameras, est, masks


def same_bits(got, want, keys, what):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {k}: {got[k]} vs {want[k]}"


def test_an_estimate_gets_the_same_bits_alone_and_in_any_company_and_chunking():
    from gigapose_amd import maskfit, refine, verify

    models, cameras, est, masks = scene()
    rgb = {k: dict(cam_K=c["cam_K"], size=(vc.H, vc.W)) for k, c in cameras.items()}     # an estimate alone may have no mask to learn the size from
    runs = (("DepthRefiner", lambda **kw: refine.DepthRefiner(models, cameras, iters=3, **kw), lambda r, e, m: r.refine(e),
             ("R", "t", "status", "inliers", "covered", "rms")),
            ("HypothesisVerifier", lambda **kw: verify.HypothesisVerifier(models, cameras, **kw), lambda r, e, m: r.score(e, m),
             ("counts", "verify_status", "verify", "depth_fit", "iou", "residual")),
            ("HypothesisVerifier, masks only", lambda **kw: verify.HypothesisVerifier(models, rgb, **kw), lambda r, e, m: r.score(e, m),
             ("counts", "verify_status", "verify", "depth_fit", "iou", "residual")),
            ("MaskRefiner", lambda **kw: maskfit.MaskRefiner(models, rgb, iters=3, **kw), lambda r, e, m: r.refine(e, m),
             ("R", "t", "maskfit_status", "iou_start", "iou", "best_iteration", "moments", "iou_counts")))
    for name, make, call, keys in runs:
        alone = [call(make(), [e], [m])[0] for e, m in zip(est, masks)]
        assert len({np.asarray(a[keys[0]]).tobytes() for a in alone}) > 6, name                    # the estimates do differ
        for per_call in (1, 2, None):
            together = call(make(pairs_per_call=per_call), est, masks)
            assert len(together) == len(est)
            for i, (got, want) in enumerate(zip(together, alone)):
                same_bits(got, want, keys, f"{name}, pairs_per_call = {per_call}: estimate {i}")
                assert got["score"] == est[i]["score"] and got["obj_id"] == est[i]["obj_id"]
