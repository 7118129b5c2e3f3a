"""Shaded rendering measurement (needs one MI355X): one object, 162 views at 480 x 640.

Workload: an icosphere of 20 480 faces painted one grey, at the level-1 template poses (tests/golden/template_poses_level1.npy,
translation x 0.4, scaled to the object's radius), under the reference's eight lights.  20 repetitions after 3 warm-ups, the
stages alternating inside every repetition, timed with HIP events (the method of tools/probe_texture.py).
  normals      : gpl_vertex_normals, two launches
  project      : gpr_project
  raster       : gpr_raster
  shade_smooth : gpl_shade, GPL_SMOOTH, 8 lights, sRGB tables of 4096 levels
  shade_flat   : gpl_shade, GPL_FLAT, the same
  shade_0      : gpl_shade, GPL_SMOOTH, no light: what the key, the triangle set-up and the colour cost
  resolve_col  : gpr_resolve on the SAME keys, for comparison
  item         : ShadedMeshTemplates.__getitem__ -- upload of the mesh, normals, the three stages, alpha boxes + crops
Nothing here is a bound: the figures are recorded, not asserted (view 0 of a smaller icosphere is checked against the numpy
restatement bit for bit, and that check does fail the run).  Writes the figures to --out (default
profiles/shade_templates.txt)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapose_amd import onboard, render, shade  # noqa: E402
from gigapose_testing import meshes  # noqa: E402
from gigapose_testing import shade_ref as sr  # noqa: E402
from gigapose_testing.probe_timing import commit, line, measure  # noqa: E402

DEV = "cuda"
H, W = 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_templates.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_shade needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    base = np.load(os.path.join(ROOT, "tests", "golden", "template_poses_level1.npy"))
    N = len(base)
    radius = 50.0                                                    # millimetres
    v, f, _ = meshes.icosphere(5, radius)
    c = np.full((len(v), 3), 102, np.uint8)
    poses = render.template_object_poses(base)
    poses[:, :3, 3] *= radius / 100.0
    poses = poses.astype(np.float32)
    lights = shade.blenderproc_lights(1000.0)
    tables = shade.srgb_tables(4096)
    say(f"device: {torch.cuda.get_device_name(0)}   commit: {args.commit or commit()}")
    say(f"workload: icosphere, {len(f)} faces, {len(v)} vertices, one grey, {N} views {H} x {W}, level-1 template poses, camera at 4 radii, "
        f"the reference's 8 lights (model units: mm), sRGB tables of {len(tables[1])} levels; {args.reps} repetitions after {args.warmup} warm-ups, "
        "stages alternating, HIP events")
    dv, df, dc, dp = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (v, f, c, poses))
    decode, encode = (torch.from_numpy(t).to(DEV) for t in tables)
    K = render._k9(onboard.TEMPLATE_K)
    xy, z = render.project(dv, dp, K, 1e-3)
    vis = torch.empty(N, H, W, dtype=torch.int64, device=DEV)
    clipped = torch.empty(N, dtype=torch.int32, device=DEV)
    unlit = torch.empty(N, dtype=torch.int32, device=DEV)
    work = torch.empty(-(-int(render.lib().gpr_raster_workspace_bytes(N, len(f))) // 8), dtype=torch.int64, device=DEV)
    rgba = torch.empty(N, H, W, 4, dtype=torch.uint8, device=DEV)
    rgba_col = torch.empty_like(rgba)
    depth = torch.empty(N, H, W, dtype=torch.float32, device=DEV)
    unit = shade.normal_unit(v)
    bufs = shade.vertex_normals_raw(dv, df, unit)
    normals = bufs[2]
    dataset = shade.ShadedMeshTemplates([((v, f, None), poses)], device=DEV)

    def lit(mode, rows):
        return lambda: shade.shade(vis, xy, z, df, dc, dv, normals, dp, K, rows, 0.0, decode, encode, mode, out=(rgba, depth, unlit))

    stages = {"normals": lambda: shade.vertex_normals_raw(dv, df, unit, out=bufs),
              "project": lambda: render.project(dv, dp, K, 1e-3, out=(xy, z)),
              "raster": lambda: render.raster(xy, z, df, H, W, out=(vis, clipped), workspace=work),
              "shade_0": lit("smooth", None),
              "shade_flat": lit("flat", lights),
              "shade_smooth": lit("smooth", lights),
              "resolve_col": lambda: render.resolve(vis, xy, z, df, dc, out=(rgba_col, depth)),
              "item": lambda: dataset[0]}
    for fn in stages.values():
        fn()
    t = measure(stages, args.reps, args.warmup)
    covered = int((rgba[..., 3] == 255).sum().item())
    levels = len(torch.unique(rgba[..., 0][rgba[..., 3] == 255]))
    say()
    say(f"{covered} covered pixels of {N * H * W} ({covered / (N * H * W):.1%}), clipped {int(clipped.sum().item())}, unlit {int(unlit.sum().item())}, "
        f"{levels} grey levels inside the masks (the unshaded render has 1); per object ({N} views):")
    say(line("normals", t["normals"], f"gpl_vertex_normals: {len(f)} faces, 9 integer atomic adds each; {len(v)} vertices"))
    say(line("project", t["project"], f"{N * len(v)} vertices"))
    say(line("raster", t["raster"], f"{N * H * W * 8 / 1e6:.0f} MB of keys initialised, {N * len(f)} triangles set up"))
    say(line("shade_smooth", t["shade_smooth"], f"gpl_shade, smooth, 8 lights: {N * H * W * 8 / 1e6:.0f} MB read, {N * H * W * 8 / 1e6:.0f} MB written"))
    say(line("shade_flat", t["shade_flat"], "gpl_shade, flat, 8 lights"))
    say(line("shade_0", t["shade_0"], "gpl_shade, smooth, no light"))
    say(line("resolve_col", t["resolve_col"], "gpr_resolve on the same keys"))
    say(line("item", t["item"], "ShadedMeshTemplates.__getitem__: upload, normals, three stages, alpha boxes + crops (with its host synchronisations)"))
    med = {k: float(np.median(x)) for k, x in t.items()}
    say(f"   normals + project + raster + shade_smooth = {(med['normals'] + med['project'] + med['raster'] + med['shade_smooth']) / 1e3:.2f} ms per object (sum of the medians)")
    say(f"   gpl_shade / gpr_resolve = {med['shade_smooth'] / med['resolve_col']:.2f} (smooth), {med['shade_flat'] / med['resolve_col']:.2f} (flat), "
        f"{med['shade_0'] / med['resolve_col']:.2f} (no light)")
    say("   per covered pixel and light the shader adds 3 subtractions, two dot products, one float64 root with its two fused tests and one")
    say(f"   float64 division; uncovered pixels ({1 - covered / (N * H * W):.0%} of the frame) leave after the key in both kernels.")
    # correctness of what was timed: a smaller icosphere (the restatement loops per face), view 0
    v2, f2, _ = meshes.icosphere(3, radius)
    c2 = np.full((len(v2), 3), 102, np.uint8)
    n2 = sr.vertex_normals(v2, f2, shade.normal_unit(v2))[2]
    want = sr.render(v2, f2, c2, n2, poses[:1], onboard.TEMPLATE_K, H, W, 1e-3, lights, 0.0, tables[0], tables[1], sr.SMOOTH)
    r = shade.ShadedMeshRenderer(H, W, onboard.TEMPLATE_K, 1e-3, lights, 0.0, tables, "smooth")
    got = r(*(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (v2, f2, c2)), dp[:1])
    same = got["rgba"].cpu().numpy().tobytes() == want["rgba"].tobytes() and got["depth"].cpu().numpy().tobytes() == want["depth"].tobytes()
    say()
    say(f"view 0 of the 1 280-face icosphere under the same lights equals the numpy restatement bit for bit: {same}")
    say("not measured, here or anywhere: the effect of these renders on pose accuracy (no trained weights, no T-LESS data), and their")
    say("distance from a Cycles render of the same scene (the model is diffuse only: DESIGN.md section 9)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
