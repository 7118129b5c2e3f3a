"""Rendering measurement (needs one MI355X): one object, 162 views at 480 x 640, kernel by kernel.

Workloads: an icosphere of 20 480 faces (a scanned model's regime: triangles of a few pixels, the one-thread-per-triangle launch)
and the 12-face box (a CAD model's regime: every triangle goes to the workgroup-per-triangle launch), both at the level-1
template poses (tests/golden/template_poses_level1.npy, translation x 0.4, scaled to the object's radius).  20 repetitions
after 3 warm-ups, the stages alternating inside every repetition, timed with HIP events.
  project : gpr_project, N*V vertices
  raster  : gpr_raster -- the memsets of the visibility buffer (N*H*W*8 bytes) and the counters, the small-triangle launch, the
            listed-triangle launch
  resolve : gpr_resolve, reads the keys and writes N*H*W*(4 + 4) bytes
  crop    : libgigapose_onboard.so on the renders (alpha boxes + crops), the stage that follows
Nothing here is a bound: the figures are recorded, not asserted (view 0 is checked against the numpy restatement bit for bit,
and that check does fail the run).  Writes the figures to --out (default profiles/render_templates.txt)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import onboard, render  # noqa: E402
from gigapose_testing import meshes, raster_ref  # noqa: E402
from gigapose_testing.probe_timing import measure  # noqa: E402
from gigapose_testing.probe_timing import line as timing_line  # noqa: E402

DEV = "cuda"
H, W = 480, 640


def line(name, v, what):
    return timing_line(name, v, what, width=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_templates.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_render needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    base = np.load(os.path.join(ROOT, "tests", "golden", "template_poses_level1.npy"))
    N = len(base)
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"workload: one object, {N} views {H} x {W}, level-1 template poses, camera at 4 radii; {args.reps} repetitions after "
        f"{args.warmup} warm-ups, stages alternating, HIP events; small-triangle threshold {render.small_triangle_pixels()} pixels")
    ok = True
    radius = 50.0
    for name, (v, f, c) in (("icosphere, 20480 faces", meshes.icosphere(5, radius)),
                            ("box, 12 faces", meshes.box((1.6 * radius, 1.0 * radius, 0.7 * radius)))):
        poses = render.template_object_poses(base)
        poses[:, :3, 3] *= radius / 100.0
        poses = poses.astype(np.float32)
        dv, df, dc, dp = (torch.from_numpy(a).to(DEV) for a in (v, f, c, poses))
        K = render._k9(onboard.TEMPLATE_K)
        xy, z = render.project(dv, dp, K, 1e-3)
        vis = torch.empty(N, H, W, dtype=torch.int64, device=DEV)
        clipped = torch.empty(N, dtype=torch.int32, device=DEV)
        work = torch.empty(-(-int(render.lib().gpr_raster_workspace_bytes(N, len(f))) // 8), dtype=torch.int64, device=DEV)
        rgba = torch.empty(N, H, W, 4, dtype=torch.uint8, device=DEV)
        depth = torch.empty(N, H, W, dtype=torch.float32, device=DEV)
        onboarder = onboard.TemplateOnboarder()
        crops = {"rgb": torch.empty(N, 3, 224, 224, device=DEV), "mask": torch.empty(N, 224, 224, device=DEV), "M": torch.empty(N, 3, 3, device=DEV)}
        stages = {"project": lambda: render.project(dv, dp, K, 1e-3, out=(xy, z)),
                  "raster": lambda: render.raster(xy, z, df, H, W, out=(vis, clipped), workspace=work),
                  "resolve": lambda: render.resolve(vis, xy, z, df, dc, out=(rgba, depth)),
                  "crop": lambda: onboarder(rgba, out=crops)}
        for fn in stages.values():
            fn()
        t = measure(stages, args.reps, args.warmup)
        listed = int(work[0].item())
        covered = int((rgba[..., 3] == 255).sum().item())
        say()
        say(f"{name}: {len(v)} vertices, {N * len(f)} (view, triangle) pairs, {listed} of them listed for the workgroup launch, "
            f"{covered} covered pixels of {N * H * W}, clipped {int(clipped.sum().item())}")
        say(line("project", t["project"], f"{N * len(v)} vertices"))
        say(line("raster", t["raster"], f"{N * H * W * 8 / 1e6:.0f} MB of keys initialised, {N * len(f)} triangles set up"))
        say(line("resolve", t["resolve"], f"{N * H * W * 8 / 1e6:.0f} MB read, {N * H * W * 8 / 1e6:.0f} MB written"))
        say(line("crop", t["crop"], "alpha boxes + crops of the same renders (libgigapose_onboard.so, with its host synchronisation)"))
        total = sum(float(np.median(t[k])) for k in ("project", "raster", "resolve"))
        say(f"   project + raster + resolve = {total / 1e3:.2f} ms per object (sum of the medians)")
        want = raster_ref.render(v, f, c, poses[:1], onboard.TEMPLATE_K, H, W, 1e-3) if len(f) <= 32768 else None
        if want is not None:
            same = rgba[:1].cpu().numpy().tobytes() == want["rgba"].tobytes() and depth[:1].cpu().numpy().tobytes() == want["depth"].tobytes()
            say(f"   view 0 equals the numpy restatement bit for bit: {same}")
            ok &= same
    say()
    say("to read these against: profiles/onboard_templates.txt records 3.6 ms per object for upload + alpha + crop of 162 finished renders")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
