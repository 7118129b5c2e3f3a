"""Writes tests/golden/rle_masks.npz: the run-length lists the UNMODIFIED reference encoder (src/utils/mask.py:mask_to_rle, loaded
from the reference tree where it lies: oracle/ref_shim.py's REFERENCE_ROOT) produces for the masks the ingest tests use.
Run once in the build container; no GPU test reads the reference tree, they read this file.

Masks: the ten 480 x 640 ellipses of synthetic.detection_case(401), then the cases none of those covers (all ten start with a
zero run): pixel (0,0) set (counts[0] == 0), all zero ([H*W]), all one ([0, H*W]), a mask with a hole, and a 37 x 53
salt-and-pepper mask.  Stored: counts (concatenated int32), offsets (int32[n+1]), sizes (int32 (n,2): H, W), names, and the
packed bits of every mask (np.packbits of the row-major mask) so that the decoder test needs nothing else."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_testing import synthetic as syn  # noqa: E402
from oracle.ref_shim import REFERENCE_ROOT  # noqa: E402

SEED = 401


def extra_masks():
    H, W = 480, 640
    yy, xx = np.mgrid[0:H, 0:W]
    first = np.zeros((H, W), np.uint8)
    first[:7, :5] = 1                                   # pixel (0, 0) set: the list starts with an empty zero run
    ring = (((xx - 300) / 200.0) ** 2 + ((yy - 240) / 150.0) ** 2 <= 1.0) & ~(((xx - 320) / 60.0) ** 2 + ((yy - 250) / 40.0) ** 2 <= 1.0)
    salt = (np.random.RandomState(SEED).rand(37, 53) < 0.5).astype(np.uint8)
    return [("first_pixel_set", first), ("all_zero", np.zeros((H, W), np.uint8)), ("all_one", np.ones((H, W), np.uint8)),
            ("hole", ring.astype(np.uint8)), ("salt_and_pepper_37x53", salt)]


def masks():
    case = syn.detection_case(SEED)
    out = [(f"ellipse_{d}", m.astype(np.uint8)) for d, m in enumerate(case["masks"])]
    return out + extra_masks()


def main():
    spec = importlib.util.spec_from_file_location("reference_mask", os.path.join(REFERENCE_ROOT, "src", "utils", "mask.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    counts, offsets, sizes, names, bits = [], [0], [], [], []
    for name, m in masks():
        rle = ref.mask_to_rle(m)
        assert rle["size"] == list(m.shape) and sum(rle["counts"]) == m.size
        counts += [int(c) for c in rle["counts"]]
        offsets.append(len(counts))
        sizes.append(m.shape)
        names.append(name)
        bits.append(np.packbits(m.ravel()))
    out = os.path.join(ROOT, "tests", "golden", "rle_masks.npz")
    np.savez_compressed(out, seed=SEED, counts=np.asarray(counts, np.int32), offsets=np.asarray(offsets, np.int32),
                        sizes=np.asarray(sizes, np.int32), names=np.asarray(names), bits=np.concatenate(bits),
                        bit_offsets=np.cumsum([0] + [len(b) for b in bits]).astype(np.int64))
    print(out, os.path.getsize(out), "bytes;", len(names), "masks;", len(counts), "runs; runs per mask:", np.diff(offsets).tolist())


if __name__ == "__main__":
    main()
