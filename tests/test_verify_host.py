"""CPU: the host half of hypothesis verification (gigapose_amd/verify.py, libgigapose_verify.so, include/gigapose_verify.h).

The numpy restatement of the header (gigapose_testing/verify_ref.py) is what the kernel is held to bit for bit
(tests/test_gpu_verify.py); here it is held to things that cannot share its mistakes: a pixel-by-pixel reading in Python sets
over a dense mask decoded by a plain loop, on planted keys and depths where every comparison is exact; and what a verifier is
for -- on the scene of refine_cases (the three-box object at its two ground truths in front of a wall, integer depths) it must
rank right hypotheses above wrong ones before and after refinement with depth only, a mask only and both, tell a surface that
floats in front of the scene from one hidden behind it, forgive an occluder the mask leaves out, and select a right hypothesis
where the coarse top-1 is wrong.  Six subtly wrong verifiers fail these checks.  Beside that: the library against its header,
the argument validation of every entry point (no GPU needed), the csv reader.

The instances are the two ground truths the scene has (refine_cases.GT, GT2), six hypotheses each: wrong_starts (90 and 180
degrees off) and starts.  An unrefined hypothesis is verified with tol = 0.25 diameters, the refiner's gate: the right starts
are up to 20 units (0.17 diameters) off along the ray, so the default 0.05 cannot recognise them and is what a REFINED
hypothesis is verified with."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

from gigapose_amd import _lib, evaluate, inout, refine, verify
from gigapose_testing import raster_ref, verify_ref
from gigapose_testing import refine_cases as rc
from gigapose_testing import verify_cases as cases
from gigapose_testing.symbols import exported_symbols

H, W = cases.H, cases.W


# ---------------------------------------------------------------------------------------------- the library and its header
def test_verify_library_exports_exactly_its_header_with_its_types():
    side = _lib.SideLibrary("libgigapose_verify.so", "gpv")       # a handle of its own: nothing but the loader has touched it
    protos = _lib.declared(side.header)
    assert side.header == "gigapose_verify.h" and side.path == verify.VERIFY_LIB_PATH
    assert sorted(protos) == ["gpv_abi_version", "gpv_counts", "gpv_last_error", "gpv_pixels_per_workgroup"]
    exported = exported_symbols(side.path)
    assert [n for n in exported if n.startswith("gpv_")] == sorted(protos)
    for prefix in ("gp_", "gpi_", "gpo_", "gps_", "gpr_", "gpt_", "gpe_", "gpd_", "gpf_"):
        assert not [n for n in exported if n.startswith(prefix)], f"a {prefix}* symbol in the verify library"
    lib = side.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    P, I = ctypes.c_void_p, ctypes.c_int
    assert lib.gpv_last_error.restype is ctypes.c_char_p
    assert list(lib.gpv_counts.argtypes) == [P, P, I, P, P, P, I, I, P, P, P, I, I, I, P, P, P]
    assert lib.gpv_abi_version() >= 1
    C = lib.gpv_pixels_per_workgroup()
    assert C == verify.pixels_per_workgroup() and C % 64 == 0 and 2 * C + 1 <= H * W      # the GPU tests place boxes around C and 2C
    for name in ("COUNTS", "UNMEASURED", "AGREE", "BEHIND", "FRONT", "UNCOVERED_IN_MASK", "RESIDUAL", "BAD_FRAME", "BAD_MASK"):
        assert getattr(verify_ref, name) == getattr(verify, name), name
    assert verify_ref.QUANTUM == 2.0 ** verify.QUANTUM_BITS
    header = open(_lib.INCLUDE_DIR + "/gigapose_verify.h").read()
    for name, value in (("GPV_COUNTS", 16), ("GPV_UNMEASURED", 0), ("GPV_AGREE", 1), ("GPV_BEHIND", 2), ("GPV_FRONT", 3), ("GPV_UNCOVERED_IN_MASK", 8),
                        ("GPV_RESIDUAL", 9), ("GPV_QUANTUM_BITS", 20), ("GPV_BAD_FRAME", 1), ("GPV_BAD_MASK", 2)):
        assert f"#define {name} {value}" in header and getattr(verify, name[4:]) == value, name


def test_verify_argument_validation_of_the_library_needs_no_gpu():
    lib = verify.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)           # `one`: a non-null pointer that is never followed
    err = lib.gpv_last_error
    names = ["vis", "depth", "frame", "cum", "offsets", "det", "box", "tol", "counts", "status"]

    def call(M=1, total=10, D=2, N=3, H=96, W=128, **ptrs):
        p = {k: ptrs.get(k, one) for k in names}
        return lib.gpv_counts(p["vis"], p["depth"], M, p["frame"], p["cum"], p["offsets"], total, D, p["det"], p["box"], p["tol"], N, H, W,
                              p["counts"], p["status"], null)

    for name in ("vis", "box", "tol", "counts", "status", "frame", "offsets", "det"):     # each required pointer in turn
        assert call(**{name: null}) == -1 and b"gpv_counts" in err() and b"null" in err(), name
    # depth and cum may be NULL; what belongs to them is then not looked at.  Nothing is launched on this machine: a launch would
    # need a device, so the calls that pass validation are the N = 0 ones below
    for kw in (dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=2048, W=2049), dict(M=0), dict(D=-1), dict(total=-1)):
        assert call(**kw) == -1 and b"bad sizes" in err(), kw
    assert call(counts=ctypes.c_void_p(12)) == -1 and b"aligned" in err()
    assert call(vis=ctypes.c_void_p(12)) == -1 and b"aligned" in err()
    assert call(cum=one, det=null) == -1 and b"det" in err()                              # det NULL with cum given
    everything = {k: null for k in names}
    assert call(N=0, **everything) == 0 and call(N=0, H=0, **everything) == -1 and b"bad sizes" in err()   # N = 0: the sizes are still checked
    assert call(N=0, M=0, D=-1, **everything) == 0                                        # ... those of what is given: no depth, no masks here
    assert call(N=0, M=0, **dict(everything, depth=one)) == -1 and call(N=0, D=-1, **dict(everything, cum=one)) == -1


def test_verify_argument_validation_of_the_python_layer_needs_no_gpu():
    N, h, w = 2, 8, 8
    i32 = torch.int32
    a = dict(vis=torch.zeros(N, h, w, dtype=torch.int64), depth=torch.zeros(1, h, w), frame=torch.zeros(N, dtype=i32),
             masks=(torch.zeros(4, dtype=i32), torch.zeros(3, dtype=i32)), det=torch.zeros(N, dtype=i32), box=torch.zeros(N, 4, dtype=i32),
             tol=torch.ones(N, dtype=torch.float64))
    for what, bad in (("vis", a["vis"].int()), ("depth", a["depth"][:, :4]), ("depth", a["depth"].double()), ("frame", a["frame"].long()),
                      ("frame", a["frame"][:1]), ("det", a["det"].long()), ("det", a["det"][:1]), ("box", a["box"][:, :3]), ("box", a["box"].long()),
                      ("tol", a["tol"].float()), ("tol", a["tol"][:1])):
        with pytest.raises(ValueError, match=what):
            verify.counts(**dict(a, **{what: bad}))
    for what, bad in (("cum", (a["masks"][0].long(), a["masks"][1])), ("offsets", (a["masks"][0], a["masks"][1].reshape(1, 3))),
                      ("offsets", (a["masks"][0], a["masks"][1][:0])), ("masks", a["masks"][0])):
        with pytest.raises(ValueError, match=what):
            verify.counts(**dict(a, masks=bad))
    with pytest.raises(ValueError, match="must be a torch tensor"):
        verify.counts(**dict(a, box=a["box"].numpy()))
    with pytest.raises(ValueError, match="2\\^22"):
        verify.counts(**dict(a, vis=torch.empty(N, 2048, 2049, dtype=torch.int64), depth=None))
    for kw in ({}, dict(depth=None, frame=None), dict(masks=None, det=None)):
        with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
            verify.counts(**dict(a, **kw))
    models = {1: dict(vertices=np.zeros((5, 3), np.float32), faces=np.zeros((4, 3), np.int32), diameter=10.0)}
    cameras = {(1, 1): dict(cam_K=cases.K, depth=np.zeros((8, 8), np.float32))}
    for kw, match in ((dict(tol=-1.0), "tol"), (dict(box="tight"), "box"), (dict(min_points=2.5), "min_points"), (dict(occlusion_weight=2.0), "occlusion_weight")):
        with pytest.raises(ValueError, match=match):
            verify.HypothesisVerifier(models, cameras, **kw)
    with pytest.raises(ValueError, match="no cameras"):
        verify.HypothesisVerifier(models, {})
    with pytest.raises(ValueError, match="diameter"):
        verify.HypothesisVerifier({1: dict(models[1], diameter=None)}, cameras)
    with pytest.raises(ValueError, match="differ in size"):
        verify.HypothesisVerifier(models, {**cameras, (1, 2): dict(cam_K=cases.K, depth=np.zeros((8, 9), np.float32))})
    with pytest.raises(ValueError, match="for every frame or for none"):
        verify.HypothesisVerifier(models, {**cameras, (1, 2): dict(cam_K=cases.K)})
    v = verify.HypothesisVerifier(models, cameras, device="cpu")
    est = dict(scene_id=1, im_id=1, obj_id=1, score=0.5, R=np.eye(3), t=np.asarray([0.0, 0.0, 100.0]), instance_id=0)
    seg = dict(size=[8, 8], counts=[10, 20, 34])
    with pytest.raises(ValueError, match="no camera"):
        v.score([dict(est, im_id=2)])
    with pytest.raises(ValueError, match="no model"):
        v.score([dict(est, obj_id=2)])
    with pytest.raises(ValueError, match="2 masks for 1"):
        v.score([est], [seg, seg])
    with pytest.raises(ValueError, match="does not match the frame size"):
        v.score([est], [dict(seg, size=[8, 9])])
    with pytest.raises(ValueError, match="polygons"):
        v.score([est], {0: [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]})
    with pytest.raises(ValueError, match="instance_id"):
        v.score([{k: x for k, x in est.items() if k != "instance_id"}], {0: seg})
    with pytest.raises(ValueError, match="score must be"):
        v.select([est], score="fine")
    for masks in (None, [seg], {0: seg}):
        with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
            v.score([est], masks)
    rgb = verify.HypothesisVerifier(models, {(1, 1): dict(cam_K=cases.K)}, device="cpu")          # the RGB-only case
    with pytest.raises(ValueError, match="masks are required"):
        rgb.score([est])
    with pytest.raises(_lib.GigaPoseHipError, match="no CPU fallback"):
        rgb.score([est], [seg])
    assert (rgb.H, rgb.W) == (8, 8)                                                               # ... takes the frame size from the masks
    assert v.pairs_per_call == min(65535, (1 << 30) // (8 * 8 * 8)) and verify.HypothesisVerifier(models, cameras, pairs_per_call=2).pairs_per_call == 2


# ---------------------------------------------------------------------------------------------- an independent reading
def dense_mask(runs, h, w):
    """A plain loop over the runs: alternating zeros and ones over the mask flattened column-major."""
    flat, value = [], 0
    for c in runs:
        flat.extend([value] * int(c))
        value ^= 1
    assert len(flat) == h * w
    return [[flat[x * h + y] for x in range(w)] for y in range(h)]            # [y][x]


def read_in_sets(keys, depth, mask, tol):
    """{slot: set of (x, y)} of one frame, pixel by pixel in Python floats (exact on the planted values); depth None: no image."""
    sets = {}
    h, w = len(mask), len(mask[0])
    for y in range(h):
        for x in range(w):
            key, bit = int(keys[y][x]), int(mask[y][x])
            if key == 2 ** 64 - 1:
                if bit:
                    sets.setdefault(8, set()).add((x, y))
                continue
            cls = 0
            if depth is not None:
                zr = struct.unpack("<f", struct.pack("<I", key >> 32))[0]
                dm = float(depth[y][x])
                if dm > 0 and dm != float("inf"):                                # false for a NaN
                    r = dm - zr
                    cls = 1 if abs(r) <= tol else 2 if r > tol else 3 if r < -tol else 0
            sets.setdefault(2 * cls + bit, set()).add((x, y))
    return sets


def per_pixel(keys, depth, runs, tol, variant=None):
    """The restatement asked pixel by pixel (1 x 1 boxes) -> {slot: set of (x, y)}, and its row for the whole frame."""
    h, w = keys.shape
    cum, offsets = (None, None) if runs is None else (np.cumsum(runs), [0, len(runs)])
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    boxes = np.stack([xs.ravel(), ys.ravel(), xs.ravel(), ys.ravel()], axis=1)
    n = len(boxes)
    d = None if depth is None else depth[None]
    rows, status = verify_ref.counts(np.broadcast_to(keys, (n, h, w)), d, np.zeros(n, np.int32), cum, offsets, np.zeros(n, np.int32), boxes,
                                     np.full(n, tol), variant)
    assert not status.any() and (rows[:, :9].sum(axis=1) <= 1).all()
    sets = {}
    for (x, y, _, _), row in zip(boxes.tolist(), rows):
        for slot in np.flatnonzero(row[:9]):
            sets.setdefault(int(slot), set()).add((x, y))
    whole, _ = verify_ref.counts(keys[None], d, [0], cum, offsets, [0], [[0, 0, w - 1, h - 1]], [tol], variant)
    return sets, whole[0]


def planted(variant=None):
    """Every kind of planted pixel with the mask bit 0 and 1 on a 7 x 12 frame -> does the restatement read what the sets read?"""
    h, w = 7, 12
    kinds = len(cases.planted_pixels())
    rs = np.random.RandomState(4)
    places = rs.permutation(h * w)[:2 * kinds]
    items = [(int(p % w), int(p // w), i % kinds, i // kinds) for i, p in enumerate(places)]
    keys, depth, mask, want = cases.planted_frame(h, w, items)
    runs = cases.mask_to_rle_counts(mask)
    assert dense_mask(runs, h, w) == mask.astype(int).tolist()
    sets = read_in_sets(keys.tolist(), depth.tolist(), mask.tolist(), cases.PLANT_TOL)
    assert sets == want and sorted(sets) == list(range(9)), "the planted frame does not hold what it says"
    got, whole = per_pixel(keys, depth, runs, cases.PLANT_TOL, variant)
    ok = got == sets and whole[:9].tolist() == [len(sets[s]) for s in range(9)]
    # the residual: of the agreeing pixels, |r| / tol = 2.25 / 6.5 (rounded), 0, 1 and 1, with either mask bit
    want9 = 2 * (round(2.25 / 6.5 * 2 ** 20) + 0 + 2 ** 20 + 2 ** 20)
    ok = ok and int(whole[9]) == want9 and not whole[10:].any()
    # no depth image: every covered pixel is unmeasured; no mask: every bit is 0
    nodepth, row = per_pixel(keys, None, runs, cases.PLANT_TOL, variant)
    ok = ok and nodepth == read_in_sets(keys.tolist(), None, mask.tolist(), cases.PLANT_TOL) and sorted(nodepth) == [0, 1, 8] and row[9] == 0
    nomask, _ = per_pixel(keys, depth, None, cases.PLANT_TOL, variant)
    ok = ok and nomask == read_in_sets(keys.tolist(), depth.tolist(), np.zeros_like(mask).tolist(), cases.PLANT_TOL) and sorted(nomask) == [0, 2, 4, 6]
    # tol = 0 with r = 0 agrees and adds no residual; tol NaN measures nothing
    zero, row0 = per_pixel(keys, depth, runs, 0.0, variant)
    exact = {(x, y) for x, y, i, _ in items if cases.planted_pixels()[i][0] == "agree exactly"}
    ok = ok and zero.get(2, set()) | zero.get(3, set()) == exact and row0[9] == 0 and zero == read_in_sets(keys.tolist(), depth.tolist(), mask.tolist(), 0.0)
    nan, rown = per_pixel(keys, depth, runs, float("nan"), variant)
    return ok and sorted(nan) == [0, 1, 8] and rown[9] == 0


def column_edges(variant=None):
    """H != W, runs of ones that begin at the first pixel of a column, end at the last pixel of one, pass from the last pixel of a
    column into the first of the next, and a mask whose very first and very last pixel are set."""
    h, w = 5, 9
    mask = np.zeros((h, w), bool)
    mask[:, 2] = True                              # a whole column: from its first to its last pixel
    mask[4, 4], mask[0, 5] = True, True            # the last pixel of column 4 and the first of column 5: one run
    mask[0, 0], mask[4, 8] = True, True            # the first and the last pixel of the mask
    mask[0, 7], mask[4, 6] = True, True            # a run of one at the first / last pixel of a column
    runs = cases.mask_to_rle_counts(mask)
    assert runs[0] == 0 and dense_mask(runs, h, w) == mask.astype(int).tolist()
    keys = np.full((h, w), raster_ref.EMPTY_KEY, np.uint64)
    keys[::2, ::2] = cases.key_of(300.0)
    depth = np.full((h, w), 301.0, np.float32)
    got, _ = per_pixel(keys, depth, runs, cases.PLANT_TOL, variant)
    return got == read_in_sets(keys.tolist(), depth.tolist(), mask.tolist(), cases.PLANT_TOL)


def test_restatement_equals_the_set_reading_on_planted_pixels():
    assert planted()


def test_restatement_reads_masks_column_major_at_the_ends_of_columns():
    assert column_edges()


# ---------------------------------------------------------------------------------------------- the csv reader
def test_read_hypotheses_on_both_files_of_the_writer(tmp_path):
    rs = np.random.RandomState(6)
    total = 0
    for b, n in enumerate((3, 2)):
        poses = np.tile(np.eye(4, dtype=np.float32), (n, 5, 1, 1))
        poses[:, :, :3, :] = rs.standard_normal((n, 5, 3, 4)).astype(np.float32)
        np.savez(tmp_path / f"{b}.npz", poses=poses, scores=rs.uniform(size=(n, 5)).astype(np.float32), object_id=rs.randint(1, 20, n),
                 scene_id=rs.randint(1, 5, n), im_id=rs.randint(0, 99, n), time=rs.uniform(size=n), detection_time=rs.uniform(size=n))
        total += n
    top1, multi = inout.save_predictions_from_batched_predictions(str(tmp_path), "ycbv", "gigapose", "run", False)
    for path, rows, ids in ((top1, total, list(range(total))), (multi, 5 * total, [i // 5 for i in range(5 * total)])):
        got, plain = verify.read_hypotheses(path), evaluate.read_estimates(path)
        assert len(got) == len(plain) == rows and [e["instance_id"] for e in got] == ids
        for a, b in zip(got, plain):
            assert set(a) == set(b) | {"instance_id"} and type(a["instance_id"]) is int
            assert all(a[k] == b[k] for k in ("scene_id", "im_id", "obj_id", "score")) and (a["R"] == b["R"]).all() and (a["t"] == b["t"]).all()
    assert "instance_id" in open(multi).readline() and "instance_id" not in open(top1).readline()


# ---------------------------------------------------------------------------------------------- what a verifier is for
MODES = ("depth", "mask", "both")


@functools.lru_cache(maxsize=None)
def drawn(which, what):
    """The keys of instance `which`'s poses: "before" / "after" the six hypotheses, "moved" the truth, it 0.5 diameters closer and
    it two diameters behind the wall."""
    v, f = rc.mesh("boxes")
    gt = cases.GTS[which]
    poses = {"before": lambda: cases.hypotheses(which), "after": lambda: cases.refined(which),
             "moved": lambda: np.stack([gt, cases.towards_camera(gt, 0.5), cases.towards_camera(gt, -(cases.WALL + 2.0 * cases.SCALE - gt[2, 3]) / cases.SCALE)])}[what]()
    return verify_ref.draw_poses(v, f, poses, cases.K, H, W), poses


def scored(which, what, mode, tol, variant=None, depth=None, runs=None, **kw):
    t = cases.truth(which)
    keys, poses = drawn(which, what)
    n = len(poses)
    depth = (t["depth"] if depth is None else depth)[None] if mode != "mask" else None
    masks = [t["runs"] if runs is None else runs] if mode != "depth" else None
    rows, status, s = verify_ref.score_drawn(keys, depth, np.zeros(n, np.int32), masks, np.zeros(n, np.int32), rc.whole_frame(n),
                                             np.full(n, tol * cases.SCALE), variant=variant, **kw)
    assert not status.any() and not keys[1].any()
    return rows, s


@functools.lru_cache(maxsize=None)
def checks(variant=None):
    """-> {name: passed} of the behaviour checks (a) .. (f) for the restatement or a wrong variant of it."""
    out, log = {}, {}
    v, _ = rc.mesh("boxes")
    # (a) every right hypothesis (3, 4, 5) above every wrong one (0, 1, 2)
    ok = True
    for which in range(len(cases.GTS)):
        for what, tol in (("before", cases.COARSE_TOL), ("after", cases.TOL)):
            for mode in MODES:
                s = scored(which, what, mode, tol, variant)[1]["verify"]
                log[which, what, mode] = s
                ok = ok and s[3:].min() > s[:3].max()
    out["a"] = ok
    # (b), (c): a surface that floats in front of the scene, one hidden behind the wall
    b = c = True
    for which in range(len(cases.GTS)):
        for mode in MODES:
            rows, s = scored(which, "moved", mode, cases.TOL, variant)
            log[which, "moved", mode] = s["verify"]
            b, c = b and s["verify"][1] < s["verify"][0], c and s["verify"][2] < s["verify"][0]
            if mode != "mask":
                cls = (rows[:, :8:2] + rows[:, 1:8:2])                      # per class
                b = b and cls[1].argmax() == verify_ref.BEHIND and cls[1, verify_ref.BEHIND] > cls[1].sum() - cls[1, verify_ref.BEHIND]
                c = c and cls[2].argmax() == verify_ref.FRONT and cls[2, verify_ref.FRONT] == cls[2].sum() > 0
                b = b and cls[0].argmax() == verify_ref.AGREE
    out["b"], out["c"] = b, c
    # (d) an occluder in the sensor's depth that the mask leaves out
    d = True
    for which in range(len(cases.GTS)):
        depth, _, runs = cases.occluded(which)
        lenient = scored(which, "after", "both", cases.TOL, variant, depth, runs, occlusion_weight=0.0)[1]["verify"]
        strict = scored(which, "after", "both", cases.TOL, variant, depth, runs, occlusion_weight=1.0)[1]["verify"]
        log[which, "occluded"] = (lenient, strict)
        d = d and (lenient[3:] > strict[3:]).all() and lenient[3:].min() > lenient[:3].max() and strict[3:].min() > strict[:3].max()
    out["d"] = d
    # (e), (f): the selection, where hypothesis 0 (the coarse top-1) is wrong
    e = f = True
    for which in range(len(cases.GTS)):
        _, poses = drawn(which, "after")
        s = scored(which, "after", "both", cases.TOL, variant)[1]["verify"]
        coarse = 0.9 - 0.01 * np.arange(6)                                  # descending: hypothesis 0, a wrong one, leads
        kept = verify_ref.select(s, coarse, [which] * 6, variant)
        e = e and len(kept) == 1 and kept[0] >= 3
        start = rc.deviation(v, cases.hypotheses(which)[kept[0]], cases.GTS[which])
        f = f and rc.deviation(v, poses[kept[0]], cases.GTS[which]) < 0.01 * start
        f = f and not rc.deviation(v, poses[0], cases.GTS[which]) < 0.01 * rc.deviation(v, cases.hypotheses(which)[0], cases.GTS[which])
    ties = verify_ref.select([0.5, 0.7, 0.7, 0.7, 0.2, 0.2], [0.9, 0.3, 0.6, 0.6, 0.1, 0.1], ["a", "a", "a", "a", "b", "b"], variant)
    e = e and ties == [2, 4]                                                # verify, then the coarse score, then the earlier position
    e = e and verify_ref.select([0.1, 0.2, 0.3], [0.5, 0.5, 0.5], ["b", "a", "b"], variant) == [2, 1]    # instances in their order of appearance
    out["e"], out["f"] = e, f
    out["planted"], out["columns"] = planted(variant), column_edges(variant)
    return out, log


def test_right_hypotheses_score_above_wrong_ones_before_and_after_refinement_in_three_modes():
    out, log = checks()
    for key in [k for k in log if k[1] in ("before", "after")]:
        print(key, np.round(log[key], 3))
    assert out["a"]


def test_a_surface_in_front_of_the_scene_is_behind_and_one_behind_the_wall_is_front():
    out, log = checks()
    for key in [k for k in log if k[1] == "moved"]:
        print(key, np.round(log[key], 3))
    assert out["b"] and out["c"]


def test_an_occluder_outside_the_mask_costs_nothing_at_weight_zero():
    out, log = checks()
    for key in [k for k in log if k[1] == "occluded"]:
        print(key, np.round(log[key][0], 3), np.round(log[key][1], 3))
    assert out["d"]


def test_selection_recovers_from_a_wrong_top_1():
    out, _ = checks()
    assert out["e"] and out["f"]


@pytest.mark.parametrize("variant", verify_ref.VARIANTS)
def test_the_checks_reject_wrong_verifiers(variant):
    """BEHIND and FRONT swapped; a row-major mask index; the gate as <; iou without the mask's uncovered pixels; ties to the later
    position; in_mask from the rank with < in place of <=."""
    must_fail = {"swapped": ("b", "c"), "row_major": ("columns", "planted"), "strict_gate": ("planted",), "iou_covered_only": ("c",),
                 "late_ties": ("e",), "strict_rank": ("columns", "planted")}[variant]
    out, _ = checks(variant)
    for name in must_fail:
        assert not out[name], name


class _Planted(verify.HypothesisVerifier):
    """The ranking of the real class over planted scores: score() gives what the estimates carry."""

    def __init__(self):
        pass

    def score(self, estimates, masks=None):
        return [dict(e) for e in estimates]


def test_select_and_rank_of_the_python_layer_break_ties_like_the_restatement():
    def est(i, instance, verify_, coarse, im=1):
        return dict(scene_id=1, im_id=im, obj_id=1, instance_id=instance, verify=verify_, score=coarse, tag=i)

    rows = [est(0, 7, 0.5, 0.9), est(1, 7, 0.7, 0.3), est(2, 7, 0.7, 0.6), est(3, 7, 0.7, 0.6), est(4, 2, 0.2, 0.1), est(5, 2, 0.2, 0.1),
            est(6, 7, 0.9, 0.1, im=2)]
    v = _Planted()
    assert [e["tag"] for e in v.select(rows)] == [2, 4, 6]
    want = verify_ref.select([r["verify"] for r in rows], [r["score"] for r in rows], [(r["im_id"], r["instance_id"]) for r in rows])
    assert want == [2, 4, 6]
    assert [e["tag"] for e in v.rank(rows)] == [2, 3, 1, 0, 4, 5, 6]
    assert [e["score"] for e in v.select(rows)] == [0.6, 0.1, 0.1]
    chosen = v.select(rows, score="verify")
    assert [e["score"] for e in chosen] == [0.7, 0.2, 0.9] and [e["coarse_score"] for e in chosen] == [0.6, 0.1, 0.1]
    loose = [{k: x for k, x in r.items() if k != "instance_id"} for r in rows[:3]]               # no instance_id: every row its own instance
    assert [e["tag"] for e in v.select(loose)] == [0, 1, 2]
    assert rows[2]["score"] == 0.6 and "coarse_score" not in rows[2]                              # the caller's dictionaries are not touched

    class Refiner:
        def refine(self, estimates):
            return [dict(e, verify=1.0 - e["verify"]) for e in estimates]

    assert [e["tag"] for e in verify.refine_and_select(Refiner(), v, rows)] == [0, 4, 6]


def test_verification_scores_equal_the_restatement_and_its_edge_rules():
    rs = np.random.RandomState(8)
    rows = np.zeros((40, 16), np.int64)
    rows[:, :10] = rs.randint(0, 400, (40, 10))
    rows[:5, 2:4] = rs.randint(0, 16, (5, 2))                     # fewer agreeing pixels than min_points
    rows[5, :8] = 0                                              # nothing covered
    rows[6, :10] = 0                                             # nothing at all: iou's denominator is the mask's area alone
    area = rows[:, 1:8:2].sum(axis=1) + rows[:, 8] + 0.0
    area[10:20] = np.nan                                         # pairs without a mask
    area[6] = 0.0
    status, clipped = np.zeros(40, np.int32), np.zeros(40, np.int32)
    status[7], clipped[8] = verify.BAD_MASK, 2
    for weight in (0.0, 0.25, 1.0):
        for has_depth in (True, False):
            got = verify.verification_scores(rows, area, status, clipped, 32, weight, tol=6.0, depth=has_depth)
            want = verify_ref.scores(rows, area, status, clipped, 32, weight, [6.0], has_depth)
            for k in ("verify", "depth_fit", "iou", "residual"):
                assert got[k].dtype == np.float64 and got[k].tobytes() == want[k].tobytes(), (k, weight, has_depth)
    s = verify.verification_scores(rows, area, status, clipped, tol=6.0)
    assert not s["depth_fit"][:5].any() and not s["verify"][[5, 6, 7, 8]].any() and s["iou"][6] == 0 and not s["iou"][10:20].any()
    assert (s["verify"][10:20] == s["depth_fit"][10:20]).all() and (s["verify"][20:] == s["depth_fit"][20:] * s["iou"][20:]).all()
    assert np.isnan(s["residual"][6]) and np.isfinite(s["residual"][9:]).all()
    assert verify.verification_scores(rows)["verify"].tobytes() == verify_ref.scores(rows, tol=[1.0])["verify"].tobytes()
