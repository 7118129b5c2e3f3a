"""What the GPU tests of the stages around the matcher share.  All of them (the renderers in front: tests/test_gpu_render.py,
test_gpu_texture.py, test_gpu_shade.py, test_gpu_planted_keys.py; the stages behind: test_gpu_refine.py, test_gpu_verify.py,
test_gpu_maskfit.py): the upload of a read-only case and the bit-for-bit comparison.  The renderers: a random rotation, a pose, a
grey mesh and the camera of a 240 x 320 frame.  The stages behind: the five drawn pairs."""
import functools

import numpy as np
import torch

from . import raster_ref
from . import refine_cases as rc

DEV = "cuda"
ZNEAR = 1e-3
K_SMALL = np.asarray([[300.0, 0.0, 160.0], [0.0, 302.0, 120.0], [0.0, 0.0, 1.0]], np.float32)      # for 240 x 320 frames


def on_gpu(a):
    a = np.array(a, copy=True)                                   # the shared cases are read-only arrays
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} of {got.size} values differ"


def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def pose(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def grey(v, value=102):
    return np.full((len(v), 3), value, np.uint8)


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
