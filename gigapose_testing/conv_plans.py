"""The launch plans of the IST convolutions in split numerics (gigapose_amd/csrc/gp_conv256.hip), as the tests see them.

The kernels run no fixed schedule: per launch the host picks a plan from the tile count (batch size x a constant of the layer) and the
kernel's GpSlotPlan cuts every XCD's chunk of tiles into segments.  Both are stated once, in gigapose_amd/csrc/gp_plan256.h, and this
module CALLS that code (gigapose_testing/plan256.py: the header compiled for the host), so that a test can enumerate every plan a batch size
selects and hold the kernels to it:

* conv_launch / stem_launch: gp_conv256_plan / gp_stem256_plan, what gp_conv2d_planes and gp_conv2d_stem_planes launch by -- kernel, ni,
  tiles_i, tiles_j, units per tile, par, slots_x, par_cap;
* slot_segments / launch_slots: GpSlotPlan with gp_halo_par_slots and chunk_tiles -> per slot the segments (tile, u0, u1, kind), kind in KINDS:
      dp      a whole tile of a data-parallel round
      head    the first units of a tile; the accumulator fragment is published
      whole   a whole tile
      rest    the last units of a tile: takes over (serial) or adds (parallel split) the fragments of the slots before it, runs the epilogue
      middle  is_head AND is_rest -- units from the middle of a tile cut into three or more pieces: takes over the fragment of slot p - 8
              and publishes its own (serial); a part that is neither first nor last (parallel split: published, nothing received)
* ist_layer_launches: the launches of one ResNet.forward; plan_class: the signature that tells two plans apart.

What is about the tests and not about the plan stays Python: the flags a slot waits for, the trace words, the plan classes.  BATCHES and
STAGE_SHAPES at the end are the cases of the GPU tests (tests/test_gpu_ist_batch_plans.py, tests/test_gpu_split.py);
tests/test_conv_plans.py holds them to the enumeration."""
from gigapose_testing import plan256

KINDS = ("dp", "head", "whole", "rest", "middle")


# ------------------------------------------------------------------------------------------------------------------ host side
def _launch(plan):
    if plan["refused"]:
        return None
    return dict(kernel=plan["kernel"], ni=plan["ni"], tiles_i=plan["tiles_i"], tiles_j=plan["tiles_j"], tiles=plan["tiles_i"] * plan["tiles_j"],
                upt=plan["upt"], steps_per_unit=plan["steps_per_unit"], par=plan["par"], slots_x=plan["slots_x"], par_cap=plan["par_cap"])


def conv_launch(B, H, W, Cin, Cout, KH, KW, stride, pad):
    """gp_conv2d_planes -> the launch: dict(kernel, ni, tiles_i, tiles_j, tiles, upt, steps_per_unit, par, slots_x, par_cap), or None where
    the entry point refuses the shape (GP_REQUIRE)."""
    return _launch(plan256.conv256(B, H, W, Cin, Cout, KH, KW, stride, pad))


def stem_launch(B, S, Cout):
    """gp_conv2d_stem_planes: conv_planes_kernel on all 256 slots, one kernel row (K = 7 x 32) per k-step."""
    return _launch(plan256.stem256(B, S, Cout))


# ------------------------------------------------------------------------------------------------------------------ device side
chunk_tiles = plan256.chunk_tiles


def slot_segments(p, grid, tiles, units_per_tile, dp_rounds_allowed, par_S):
    """GpSlotPlan of workgroup p of a grid of `grid`: -> [(tile, u0, u1, kind)] in the order the slot runs them."""
    segs = plan256.slot_segments(p, grid, tiles, units_per_tile, dp_rounds_allowed, par_S)
    return [(t, u0, u1, "dp" if dp else "middle" if (head and rest) else "head" if head else "rest" if rest else "whole")
            for t, u0, u1, head, rest, dp in segs]


def launch_slots(launch):
    """The kernel's side of a launch (conv_launch / stem_launch) -> dict(launch, grid=8 slots_x, slots={p: segments}, par_S={x: S of that XCD})."""
    grid, T, upt = 8 * launch["slots_x"], launch["tiles"], launch["upt"]
    slots, S_of = {}, {}
    for p in range(grid):
        x = p & 7
        par_S = 0
        if launch["par"]:                                              # conv_halo_kernel<.., PAR = true>; ncb = upt
            par_S = plan256.halo_par_slots(launch["par_cap"], grid >> 3, chunk_tiles(T, x), upt)
            S_of[x] = par_S
        slots[p] = slot_segments(p, grid, T, upt, not launch["par"], par_S)
    return dict(launch, grid=grid, slots=slots, par_S=S_of)


def handoff_wait_flags(plan, p):
    """The flags gp_handoff_wait is given by slot p before its last segment's epilogue or k loop: serial -- the flag of slot p - 8 for a rest
    or middle; parallel split -- x + 8 (n - 1) down to x + 8 m_lo (stride 8) for the owner of a tile."""
    segs = plan["slots"][p]
    if not segs or segs[-1][3] not in ("rest", "middle"):
        return []
    if not plan["par"]:
        return [p - 8]
    if segs[-1][3] == "middle":                                        # a published part: nothing is received
        return []
    x, n = p & 7, p >> 3
    par_S = plan["par_S"][x]
    m_lo = n - (par_S - 1)
    first_slot, last_slot, stride = x + 8 * (n - 1), x + 8 * m_lo, 8
    count = (first_slot - last_slot) // stride + 1
    return [first_slot - stride * i for i in range(count)]


def trace_words(plan):
    """What the probe build's trace holds per slot: (segments run, k-steps run) -- the halo kernel counts 9 k-steps per channel block."""
    return {p: (len(s), sum(u1 - u0 for _, u0, u1, _ in s) * plan["steps_per_unit"]) for p, s in plan["slots"].items()}


# ------------------------------------------------------------------------------------------------------------------ classes
def plan_class(plan):
    """The signature that tells two plans apart: (kernel, "par" | "serial", slots_x, tile count divisible by 8, segment kinds that occur,
    the par_S values of the XCDs, whether a slot has no segment)."""
    kinds = {k for s in plan["slots"].values() for *_, k in s}
    return (plan["kernel"], "par" if plan["par"] else "serial", plan["slots_x"], plan["tiles"] % 8 == 0, tuple(k for k in KINDS if k in kinds),
            tuple(sorted(set(plan["par_S"].values()))), any(not s for s in plan["slots"].values()))


def describe_class(c):
    kernel, mode, slots_x, div8, kinds, S, idle = c
    return (f"{kernel:6s} {mode:6s} slots_x={slots_x:2d} tiles%8{'==' if div8 else '!='}0 segments={'+'.join(kinds)}"
            + (f" par_S={'/'.join(map(str, S))}" if S else "") + (" idle slots" if idle else ""))


def class_features(c):
    """A class taken apart: the properties a stage-level case can have one by one (see STAGE_SHAPES)."""
    kernel, mode, slots_x, div8, kinds, S, idle = c
    f = {("kind", kernel, mode, k) for k in kinds} | {("slots_x", kernel, mode, slots_x), ("div8", kernel, mode, div8)}
    if mode == "par":
        f |= {("par_S values", len(S)), ("S=1", 1 in S), ("idle", idle)}
    return f


def ist_layer_launches(cfg, B):
    """The convolution launches of ResNet.forward in split numerics, conv_kernel "256", in launch order: [(name, launch)]: the stem, per
    BasicBlock conv1, the 1 x 1 shortcut where the block strides, conv2, and the 1 x 1 head -- 21 in all for four layers of two blocks."""
    S, c0, dims = cfg["input_size"], cfg["initial_dim"], list(cfg["block_dims"])
    out = [("stem", stem_launch(B, S, c0))]
    H = S // 2
    chans = [c0] + dims
    for i, stride in enumerate([1, 2, 2, 2]):
        for blk, (cin, s) in enumerate(((chans[i], stride), (chans[i + 1], 1))):
            cout = chans[i + 1]
            out.append((f"layer{i + 1}.{blk}.conv1", conv_launch(B, H, H, cin, cout, 3, 3, s, 1)))
            if s != 1:
                out.append((f"layer{i + 1}.{blk}.downsample", conv_launch(B, H, H, cin, cout, 1, 1, s, 0)))
            H = (H + 2 - 3) // s + 1
            out.append((f"layer{i + 1}.{blk}.conv2", conv_launch(B, H, H, cout, cout, 3, 3, 1, 1)))
    out.append(("layer4_outconv", conv_launch(B, H, H, dims[3], cfg["descriptor_size"], 1, 1, 1, 0)))
    return out


IST_CFG = dict(n_heads=0, input_dim=3, input_size=256, initial_dim=128, block_dims=[128, 192, 256, 512], descriptor_size=256)


def ist_classes(cfg, B):
    """-> {class: name of the first layer of the forward at batch size B that runs it}"""
    out = {}
    for name, launch in ist_layer_launches(cfg, B):
        assert launch is not None, (name, B)
        out.setdefault(plan_class(launch_slots(launch)), name)
    return out


def stage_launch(shape):
    cin, cout, k, stride, pad, hw, B, res = shape
    return conv_launch(B, hw, hw, cin, cout, k, k, stride, pad)


# ------------------------------------------------------------------------------------------------------------------ the cases of the GPU tests
# Batch sizes of the backbone sweep (tests/test_gpu_ist_batch_plans.py): together they run EVERY plan class that a batch size from 1 to
# 64 selects in any layer of IST_CFG.  Each entry names the classes it adds to the entries before it (describe_class); tests/test_conv_plans.py
# checks that each named class is one of that batch size and that no class of B = 1 .. 64 is left out.
BATCHES = [
    (1, (
        'gather serial slots_x= 1 tiles%8!=0 segments=whole idle slots',
        'gather serial slots_x= 2 tiles%8==0 segments=whole',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=4',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=6 idle slots',
        'halo   serial slots_x= 1 tiles%8!=0 segments=whole idle slots',
        'stem   serial slots_x=32 tiles%8==0 segments=head+rest+middle',
    )),
    (2, (
        'gather serial slots_x= 1 tiles%8==0 segments=whole',
        'gather serial slots_x= 4 tiles%8==0 segments=whole',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest par_S=2',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=8 idle slots',
        'halo   serial slots_x= 2 tiles%8!=0 segments=head+rest idle slots',
        'stem   serial slots_x=32 tiles%8==0 segments=head+rest',
    )),
    (4, (
        'gather serial slots_x= 2 tiles%8==0 segments=head+rest',
        'gather serial slots_x= 8 tiles%8==0 segments=whole',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=16 idle slots',
        'halo   serial slots_x=32 tiles%8==0 segments=whole',
        'stem   serial slots_x=32 tiles%8==0 segments=whole',
    )),
    (5, (
        'gather serial slots_x= 1 tiles%8!=0 segments=dp+whole',
        'gather serial slots_x= 2 tiles%8!=0 segments=head+whole+rest',
        'gather serial slots_x= 4 tiles%8!=0 segments=head+rest',
        'gather serial slots_x= 8 tiles%8==0 segments=head+whole+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=8 idle slots',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=16 idle slots',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=3 idle slots',
        'halo   serial slots_x=32 tiles%8==0 segments=head+whole+rest',
        'stem   serial slots_x=32 tiles%8==0 segments=head+whole+rest',
    )),
    (8, (
        'gather serial slots_x= 4 tiles%8==0 segments=head+rest',
        'gather serial slots_x=16 tiles%8==0 segments=whole',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=8',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=16',
        'halo   serial slots_x=32 tiles%8==0 segments=dp+whole',
        'stem   serial slots_x=32 tiles%8==0 segments=dp+whole',
    )),
    (11, (
        'gather serial slots_x= 4 tiles%8!=0 segments=head+whole+rest',
        'gather serial slots_x= 8 tiles%8!=0 segments=head+rest+middle',
        'gather serial slots_x=16 tiles%8==0 segments=head+whole+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=5/6 idle slots',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=10/16 idle slots',
        'halo   par    slots_x=32 tiles%8==0 segments=whole par_S=1 idle slots',
        'halo   serial slots_x=32 tiles%8==0 segments=dp+head+whole+rest',
        'stem   serial slots_x=32 tiles%8==0 segments=dp+head+whole+rest',
    )),
    (12, (
        'gather serial slots_x= 2 tiles%8==0 segments=head+whole+rest',
        'gather serial slots_x= 4 tiles%8==0 segments=head+whole+rest',
        'gather serial slots_x= 8 tiles%8==0 segments=head+rest',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=5 idle slots',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=10 idle slots',
    )),
    (14, (
        'gather serial slots_x= 2 tiles%8!=0 segments=dp+head+whole+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=8/10 idle slots',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=4 idle slots',
    )),
    (17, (
        'gather serial slots_x= 8 tiles%8!=0 segments=head+whole+rest',
        'gather serial slots_x=32 tiles%8==0 segments=head+whole+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=3/4 idle slots',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=6/8 idle slots',
    )),
    (20, (
        'gather serial slots_x= 8 tiles%8==0 segments=head+rest+middle',
        'gather serial slots_x=16 tiles%8==0 segments=head+rest+middle',
    )),
    (21, (
        'gather serial slots_x=16 tiles%8!=0 segments=head+rest+middle',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=2/3 idle slots',
    )),
    (24, (
        'gather serial slots_x=16 tiles%8==0 segments=head+rest',
        'halo   par    slots_x=32 tiles%8==0 segments=head+rest par_S=2 idle slots',
    )),
    (25, (
        'gather serial slots_x= 8 tiles%8!=0 segments=head+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest par_S=2 idle slots',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=4/5 idle slots',
    )),
    (29, (
        'gather serial slots_x= 4 tiles%8!=0 segments=dp+head+whole+rest',
        'gather serial slots_x=16 tiles%8!=0 segments=head+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=4 idle slots',
    )),
    (33, (
        'gather serial slots_x=16 tiles%8!=0 segments=head+whole+rest',
        'gather serial slots_x=32 tiles%8==0 segments=dp+head+whole+rest',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+whole+rest par_S=1/2 idle slots',
    )),
    (38, (
        'gather serial slots_x=32 tiles%8==0 segments=head+rest+middle',
        'halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=3 idle slots',
    )),
    (61, (
        'gather serial slots_x= 8 tiles%8!=0 segments=dp+head+whole+rest',
        'gather serial slots_x=32 tiles%8!=0 segments=head+rest',
        'gather serial slots_x=32 tiles%8!=0 segments=head+rest+middle',
        'halo   par    slots_x=32 tiles%8!=0 segments=whole par_S=1 idle slots',
    )),
    (63, (
        'gather serial slots_x=16 tiles%8!=0 segments=dp+head+whole+rest',
        'gather serial slots_x=32 tiles%8!=0 segments=head+whole+rest',
    )),
    (64, (
        'gather serial slots_x=32 tiles%8==0 segments=dp+whole',
        'gather serial slots_x=32 tiles%8==0 segments=head+rest',
        'gather serial slots_x=32 tiles%8==0 segments=whole',
    )),
]

# Stage-level cases of gp_conv2d_planes against float64 (tests/test_gpu_split.py), (cin, cout, k, stride, pad, hw, B, res) as
# CONV_PLANES_SHAPES there, each at the smallest shape that has its plan: the plan depends only on kernel, tile count and units per tile.
# Halo cases are 16 x 16 images (tiles = B x co-tiles), gather cases 3 x 3 / stride 2 from 32 x 32 (one pixel tile per image) or 1 x 1.
# One launch has one class and the list is held to 16 entries, so it cannot name each of the 72 classes of gp_conv2d_planes one by one
# (the 6 stem classes belong to gp_conv2d_stem_planes: tests/test_gpu_stem_planes.py and the backbone sweep).  What it is held to
# (tests/test_conv_plans.py): every PROPERTY of every class (class_features: each segment kind, each slots_x, both tile-count parities
# per kernel and mode; one and two par_S values, S = 1, idle slots or none) occurs in some entry, and every plan the list promises is
# the one the model gives.  The whole classes are the business of BATCHES.
STAGE_SHAPES = [
    ((256, 512, 3, 2, 1, 32, 15, True), "gather serial slots_x= 8 tiles%8!=0 segments=head+rest+middle",       # layer4 conv1: 30 tiles x 72 k-steps, a slot's 33-34 steps lie inside one tile; residual
     "gather middle segment, chain at slots_x = 8, residual"),
    ((256, 128, 3, 2, 1, 32, 8, False), "gather serial slots_x= 2 tiles%8==0 segments=head+rest", "gather chain at slots_x = 2"),
    ((256, 128, 3, 2, 1, 32, 17, False), "gather serial slots_x= 4 tiles%8!=0 segments=head+rest", "gather chain at slots_x = 4"),
    ((512, 128, 3, 2, 1, 32, 32, False), "gather serial slots_x=16 tiles%8==0 segments=head+rest+middle", "gather chain at slots_x = 16 (tiles of 144 k-steps in 4-5 pieces)"),
    ((64, 256, 1, 1, 0, 16, 25, False), "gather serial slots_x= 2 tiles%8!=0 segments=dp+head+whole+rest", "gather data-parallel rounds + a cut remainder on 16 slots"),
    ((64, 128, 1, 1, 0, 16, 257, False), "gather serial slots_x=32 tiles%8!=0 segments=head+whole+rest", "gather on all 256 slots, 257 tiles"),
    ((32, 128, 1, 1, 0, 16, 9, False), "gather serial slots_x= 1 tiles%8!=0 segments=dp+whole", "gather on 8 slots: whole tiles, two on one XCD"),
    ((512, 128, 3, 1, 1, 16, 7, False), "halo   serial slots_x= 2 tiles%8!=0 segments=head+rest idle slots", "halo, 7 tiles: serial on 16 slots, one XCD without a tile"),
    ((128, 64, 3, 1, 1, 16, 8, True), "halo   par    slots_x=32 tiles%8==0 segments=head+rest+middle par_S=4 idle slots", "halo parallel, 8 tiles, Cout = 64, four parts per tile, residual"),
    ((64, 64, 3, 1, 1, 16, 255, False), "halo   par    slots_x=32 tiles%8!=0 segments=whole par_S=1 idle slots", "halo parallel, 255 tiles: S = 1 and one idle slot"),
    ((64, 64, 3, 1, 1, 16, 256, False), "halo   serial slots_x=32 tiles%8==0 segments=whole", "halo, 256 tiles: one whole tile per slot"),
    ((64, 64, 3, 1, 1, 16, 257, False), "halo   serial slots_x=32 tiles%8!=0 segments=head+whole+rest", "halo serial with cut tiles, 257 tiles"),
    ((64, 64, 3, 1, 1, 16, 520, False), "halo   serial slots_x=32 tiles%8==0 segments=dp+head+whole+rest", "halo serial: a data-parallel round + a cut remainder"),
    ((128, 128, 3, 1, 1, 16, 68, False), "halo   par    slots_x=32 tiles%8!=0 segments=head+rest+middle par_S=3/4 idle slots", "halo parallel, par_S = 4 on XCDs with 8 tiles and 3 on those with 9"),
    ((64, 128, 3, 1, 1, 16, 128, True), "halo   par    slots_x=32 tiles%8==0 segments=head+rest par_S=2", "halo parallel, every slot busy, residual"),
    ((64, 128, 3, 1, 1, 16, 3, False), "halo   serial slots_x= 1 tiles%8!=0 segments=whole idle slots", "halo on 8 slots, 3 tiles"),
]
