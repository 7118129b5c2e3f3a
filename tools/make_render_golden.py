"""Copies the reference's 162 level-1 icosphere object poses (src/lib3d/predefined_poses/obj_poses_level1.npy, (162,4,4) float64,
object -> camera, translation in mm, what get_obj_poses_from_template_level(level=1, pose_distribution="all") loads) to
tests/golden/template_poses_level1.npy, unchanged: the poses tests/test_gpu_render.py renders at the real size.  Needs the
reference tree (--reference, default: the directory oracle/ref_shim.py knows); runs on the CPU, no GPU involved.
The file is data the reference reads, not code; generating the poses is out of this project's scope."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from oracle import ref_shim

    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=ref_shim.REFERENCE_ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "template_poses_level1.npy"))
    args = ap.parse_args()
    src = os.path.join(args.reference, "src", "lib3d", "predefined_poses", "obj_poses_level1.npy")
    poses = np.load(src)
    assert poses.shape == (162, 4, 4) and poses.dtype == np.float64, (poses.shape, poses.dtype)
    R, t = poses[:, :3, :3], poses[:, :3, 3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-6) and np.allclose(np.linalg.det(R), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(t, axis=1), 1000.0, atol=1e-3) and (poses[:, 3] == (0, 0, 0, 1)).all()
    np.save(args.out, poses)
    print(f"{args.out}: {poses.shape} {poses.dtype}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
