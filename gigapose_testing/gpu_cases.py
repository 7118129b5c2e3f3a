"""What the GPU tests of the stages behind the matcher (tests/test_gpu_refine.py, test_gpu_verify.py, test_gpu_maskfit.py) share:
the upload of a read-only case, the bit-for-bit comparison and the five drawn pairs."""
import functools

import numpy as np
import torch

from . import raster_ref
from . import refine_cases as rc

DEV = "cuda"


def on_gpu(a):
    a = np.array(a, copy=True)                                   # the shared cases are read-only arrays
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} of {got.size} values differ"


@functools.lru_cache(maxsize=None)
def five_pairs():
    """The three starts about GT and two about GT2 of the three-box object: (poses f64 (5,4,4), keys uint64 (5,H,W) from render.project
    + render.raster on refine_cases.K)."""
    from gigapose_amd import render

    v, f = rc.mesh("boxes")
    poses = np.concatenate([rc.starts(), np.stack([rc.moved(rc.GT2, [1, 1, 0], 5, (3, 2, -6)), rc.moved(rc.GT2, [0, 1, 2], 10, (-4, 5, 9))])])
    xy, vd = render.project(on_gpu(v), on_gpu(poses.astype(np.float32)), rc.K, 1e-3)
    vis, clipped = render.raster(xy, vd, on_gpu(f), rc.H, rc.W)
    vis = vis.cpu().numpy().view(np.uint64)
    assert not clipped.any().item() and ((vis != raster_ref.EMPTY_KEY).sum(axis=(1, 2)) > 200).all()
    poses.setflags(write=False), vis.setflags(write=False)
    return poses, vis
