"""Inputs for the tests of hypothesis verification (gigapose_amd/verify.py, gigapose_testing/verify_ref.py), shared by the CPU
and the GPU suite.  The scene is refine_cases': the three-box object and a sphere in front of a wall at 96 x 128, integer depths
as a depth PNG holds them, `starts` (right hypotheses) and `wrong_starts` (90 and 180 degrees off).  Added here: the scene's two
instances of the object (at GT and GT2, one frame each) with six hypotheses each, detection masks derived from the ground-truth silhouette and encoded with
ingest.mask_to_rle_counts, an occluder, and planted keys on which every comparison of the classification is exact."""
import functools

import numpy as np

from gigapose_amd.ingest import mask_to_rle_counts

from . import raster_ref, refine_ref, verify_ref
from . import refine_cases as rc

H, W, K, SCALE, WALL = rc.H, rc.W, rc.K, rc.SCALE, rc.WALL
TOL = 0.05                                           # HypothesisVerifier's default, x SCALE
COARSE_TOL = 0.25                                    # the refiner's gate: what a coarse pose is verified with (see test_verify_host.py)
GTS = (rc.GT, rc.GT2)                                # the ground truths refine_cases.sensor_depth draws


@functools.lru_cache(maxsize=None)
def truth(which):
    """Instance `which` (0: GT, 1: GT2) of the three-box object: its keys at the ground truth, the sensor's depth (integers, the wall behind), the
    silhouette and its run lengths."""
    v, f = rc.mesh("boxes")
    vis = rc.draw(v, f, GTS[which])
    depth = rc.depth_of(vis)
    mask = vis != raster_ref.EMPTY_KEY
    runs = mask_to_rle_counts(mask)
    for a in (vis, depth, mask, runs):
        a.setflags(write=False)
    return dict(vis=vis, depth=depth, mask=mask, runs=runs)


def segmentation(runs):
    return dict(size=[H, W], counts=[int(c) for c in runs])


def hypotheses(which):
    """Six poses of instance `which`: three wrong ones first (so that a wrong one is hypothesis 0), then the three right ones."""
    return np.concatenate([rc.wrong_starts(GTS[which]), rc.starts(GTS[which])])


def towards_camera(gt, diameters):
    """`gt` moved along its viewing ray: a positive amount brings it closer."""
    t = gt[:3, 3]
    return rc.rigid(gt[:3, :3], t - diameters * SCALE * t / np.linalg.norm(t))


@functools.lru_cache(maxsize=None)
def refined(which):
    """The restatement's refinement loop (refine_ref.refine, the defaults of DepthRefiner on the whole frame) on the six hypotheses
    of instance `which` -> poses (6,4,4); a pair that stops keeps its input pose."""
    v, f = rc.mesh("boxes")
    p = hypotheses(which)
    n = len(p)
    out = refine_ref.refine(v, f, p, np.tile(K, (n, 1)), truth(which)["depth"][None], np.zeros(n, np.int32), rc.whole_frame(n), np.full(n, rc.GATE),
                            np.full(n, SCALE), rc.ITERS, rc.STEP["min_points"], rc.STEP["min_pivot"], rc.STEP["damping"], rc.STEP["tol2"], H, W)
    out["poses"].setflags(write=False)
    return out["poses"]


def occluded(which):
    """An occluder in front of instance `which`: a vertical bar over the middle third of its silhouette's columns, 150 units
    closer than the object, drawn into the sensor's depth and cut out of the mask -> (depth, mask, run lengths)."""
    t = truth(which)
    xs = np.flatnonzero(t["mask"].any(axis=0))
    a, b = xs[0] + (xs[-1] - xs[0]) // 3, xs[0] + 2 * (xs[-1] - xs[0]) // 3
    depth, mask = t["depth"].copy(), t["mask"].copy()
    depth[:, a:b + 1] = np.float32(GTS[which][2, 3] - 150.0)
    mask[:, a:b + 1] = False
    return depth, mask, mask_to_rle_counts(mask)


# ------------------------------------------------------------------------------------------------ planted pixels
def key_of(z, face=0):
    return (np.uint64(np.asarray([z], np.float32).view(np.uint32)[0]) << np.uint64(32)) | np.uint64(face)


PLANT_TOL = 6.5                                      # dyadic: every |r| <= tol below is decided exactly
PLANT_Z = 300.0


def planted_pixels():
    """(name, drawn depth or None = uncovered, measured depth, expected class or None) of the pixels every rule needs: each class,
    |r| exactly tol on either side, one f32 step beyond on either side, and measurements that are no measurement."""
    up, down = np.float32(1e9), np.float32(0)
    f32 = np.float32
    return [("agree", PLANT_Z, f32(302.25), verify_ref.AGREE), ("agree exactly", PLANT_Z, f32(300.0), verify_ref.AGREE),
            ("behind", PLANT_Z, f32(340.0), verify_ref.BEHIND), ("front", PLANT_Z, f32(250.0), verify_ref.FRONT),
            ("at +tol", PLANT_Z, f32(306.5), verify_ref.AGREE), ("one step beyond +tol", PLANT_Z, np.nextafter(f32(306.5), up), verify_ref.BEHIND),
            ("at -tol", PLANT_Z, f32(293.5), verify_ref.AGREE), ("one step beyond -tol", PLANT_Z, np.nextafter(f32(293.5), down), verify_ref.FRONT),
            ("dm = 0", PLANT_Z, f32(0.0), verify_ref.UNMEASURED), ("dm < 0", PLANT_Z, f32(-300.0), verify_ref.UNMEASURED),
            ("dm NaN", PLANT_Z, f32(np.nan), verify_ref.UNMEASURED), ("dm +inf", PLANT_Z, f32(np.inf), verify_ref.UNMEASURED),
            ("uncovered", None, f32(300.0), None)]


def planted_frame(h, w, items):
    """An h x w frame, empty but for the planted pixels: items = [(x, y, index into planted_pixels(), mask bit)] -> keys (h,w) u64,
    depth (h,w) f32 (0 elsewhere), the dense mask (h,w) bool, and the set of (x, y) expected per slot of the counts:
    {2*class + bit, or 8 for an uncovered pixel in the mask: set}."""
    keys = np.full((h, w), raster_ref.EMPTY_KEY, np.uint64)
    depth = np.zeros((h, w), np.float32)
    mask = np.zeros((h, w), bool)
    want = {}
    pixels = planted_pixels()
    for x, y, i, bit in items:
        name, z, dm, cls = pixels[i]
        assert keys[y, x] == raster_ref.EMPTY_KEY and not mask[y, x] and depth[y, x] == 0, "two planted pixels on one place"
        if z is not None:
            keys[y, x] = key_of(z, i)
        depth[y, x], mask[y, x] = dm, bool(bit)
        if cls is not None or bit:
            want.setdefault(verify_ref.UNCOVERED_IN_MASK if cls is None else 2 * cls + bit, set()).add((x, y))
    return keys, depth, mask, want
