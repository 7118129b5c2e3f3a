"""Host model of the launch plans of the IST convolutions in split numerics (gigapose_amd/csrc/gp_conv256.hip, gp_tile256.h).

The kernels run no fixed schedule: per launch the host picks a plan from the tile count (batch size x a constant of the layer) and the
kernel's GpSlotPlan cuts every XCD's chunk of tiles into segments.  This module restates those decisions line by line, with the names of
the sources, so that a test can enumerate every plan a batch size selects and hold the kernels to it:

* conv_launch / stem_launch: gp_conv2d_planes, conv_halo_launch, gp_conv2d_stem_planes -- halo usable, ni, tiles_i, tiles_j, units per tile,
  par, the slots_x loop, par_cap;
* slot_segments / launch_slots: GpSlotPlan with par_S and chunk_tiles -> per slot the segments (tile, u0, u1, kind), kind in KINDS:
      dp      a whole tile of a data-parallel round
      head    the first units of a tile; the accumulator fragment is published
      whole   a whole tile
      rest    the last units of a tile: takes over (serial) or adds (parallel split) the fragments of the slots before it, runs the epilogue
      middle  is_head AND is_rest -- units from the middle of a tile cut into three or more pieces: takes over the fragment of slot p - 8
              and publishes its own (serial); a part that is neither first nor last (parallel split: published, nothing received)
* ist_layer_launches: the launches of one ResNet.forward; plan_class: the signature that tells two plans apart.

BATCHES and STAGE_SHAPES at the end are the cases of the GPU tests (tests/test_gpu_ist_batch_plans.py, tests/test_gpu_split.py);
tests/test_conv_plans.py holds them to the enumeration."""

CBK, CT = 32, 256
KINDS = ("dp", "head", "whole", "rest", "middle")
g_conv_par_min_cb = 1


# ------------------------------------------------------------------------------------------------------------------ host side
def conv_halo_usable(H, W, Cin, Cout, KH, KW, stride, pad):
    return KH == 3 and KW == 3 and stride == 1 and pad == 1 and H % 16 == 0 and W % 16 == 0 and Cin % 32 == 0 and Cout % 64 == 0


def conv_launch(B, H, W, Cin, Cout, KH, KW, stride, pad):
    """gp_conv2d_planes -> the launch: dict(kernel, ni, tiles_i, tiles_j, tiles, upt, steps_per_unit, par, slots_x, par_cap), or None where
    the entry point refuses the shape (GP_REQUIRE)."""
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    K = KH * KW * Cin
    npix = B * OH * OW
    if not (Cin % 32 == 0 and Cout % 64 == 0 and KH * KW <= 9 and npix % CT == 0 and B > 0):
        return None
    ni = 4 if Cout >= 256 else Cout // 64
    if conv_halo_usable(H, W, Cin, Cout, KH, KW, stride, pad):          # conv_halo_launch
        tiles_i = B * (OH // 16) * (OW // 16)
        tiles_j = (Cout + 64 * ni - 1) // (64 * ni)
        ncb = Cin // CBK
        n_tiles, units = tiles_i * tiles_j, tiles_i * tiles_j * ncb * 9
        slots_x = 32
        par = n_tiles < 8 * slots_x and n_tiles >= 8 and ncb >= 2
        par_cap = max(1, ncb // g_conv_par_min_cb)
        while (not par) and slots_x > 1 and n_tiles < 8 * slots_x and units // (8 * slots_x) < 32:
            slots_x >>= 1
        return dict(kernel="halo", ni=ni, tiles_i=tiles_i, tiles_j=tiles_j, tiles=n_tiles, upt=ncb, steps_per_unit=9, par=par, slots_x=slots_x,
                    par_cap=par_cap)
    tiles_i = npix // CT
    tiles_j = (Cout + 64 * ni - 1) // (64 * ni)
    n_tiles, units = tiles_i * tiles_j, tiles_i * tiles_j * (K // CBK)
    slots_x = 32
    while slots_x > 1 and n_tiles < 8 * slots_x and units // (8 * slots_x) < 32:
        slots_x >>= 1
    return dict(kernel="gather", ni=ni, tiles_i=tiles_i, tiles_j=tiles_j, tiles=n_tiles, upt=K // CBK, steps_per_unit=1, par=False, slots_x=slots_x,
                par_cap=1)


def stem_launch(B, S, Cout):
    """gp_conv2d_stem_planes: conv_planes_kernel on all 256 slots, one kernel row (K = 7 x 32) per k-step."""
    npix = B * (S // 2) * (S // 2)
    if not (B > 0 and S % 2 == 0 and (Cout in (128, 192) or Cout % 256 == 0) and npix % CT == 0):
        return None
    ni = 4 if Cout >= 256 else Cout // 64
    tiles_i = npix // CT
    tiles_j = (Cout + 64 * ni - 1) // (64 * ni)
    return dict(kernel="stem", ni=ni, tiles_i=tiles_i, tiles_j=tiles_j, tiles=tiles_i * tiles_j, upt=7, steps_per_unit=1, par=False, slots_x=32,
                par_cap=1)


# ------------------------------------------------------------------------------------------------------------------ device side
def chunk_tiles(tiles, x):
    return tiles * (x + 1) // 8 - tiles * x // 8


def slot_segments(p, grid, tiles, units_per_tile, dp_rounds_allowed, par_S):
    """GpSlotPlan of workgroup p of a grid of `grid`: -> [(tile, u0, u1, kind)] in the order the slot runs them."""
    x, n, slots_x = p & 7, p >> 3, grid >> 3
    upt = units_per_tile
    t_lo = tiles * x // 8
    n_t = tiles * (x + 1) // 8 - t_lo
    rounds_dp = n_t // slots_x - 1 if (dp_rounds_allowed and n_t // slots_x > 1) else 0
    n_dp = rounds_dp * slots_x
    U = (n_t - n_dp) * upt
    u0, u1 = U * n // slots_x, U * (n + 1) // slots_x
    if par_S > 0:
        tile = n // par_S
        part = n - tile * par_S
        u0 = u1 = 0
        if tile < n_t:
            u0 = tile * upt + upt * part // par_S
            u1 = tile * upt + upt * (part + 1) // par_S
    ta, sa = u0 // upt, u0 % upt
    tb, sb = u1 // upt, u1 % upt
    n_head, n_rest = (1 if sb > 0 else 0), (1 if sa > 0 else 0)
    first_whole = ta + n_rest
    n_seg = rounds_dp + n_head + (tb - first_whole) + n_rest
    segs = []
    for seg in range(n_seg):                                           # GpSlotPlan::segment
        is_dp = seg < rounds_dp
        is_head = (not is_dp) and seg - rounds_dp < n_head
        is_rest = (not is_dp) and n_rest == 1 and seg == n_seg - 1
        t = seg * slots_x + n if is_dp else n_dp + (tb if is_head else (ta if is_rest else first_whole + seg - rounds_dp - n_head))
        kind = "dp" if is_dp else "middle" if (is_head and is_rest) else "head" if is_head else "rest" if is_rest else "whole"
        segs.append((t_lo + t, sa if is_rest else 0, sb if is_head else upt, kind))
    return segs


def launch_slots(launch):
    """The kernel's side of a launch (conv_launch / stem_launch) -> dict(launch, grid=8 slots_x, slots={p: segments}, par_S={x: S of that XCD})."""
    grid, T, upt = 8 * launch["slots_x"], launch["tiles"], launch["upt"]
    slots, S_of = {}, {}
    for p in range(grid):
        x = p & 7
        par_S = 0
        if launch["par"]:                                              # conv_halo_kernel<.., PAR = true>; ncb = upt
            par_S = min(min(max(1, (grid >> 3) // max(chunk_tiles(T, x), 1)), upt), max(1, launch["par_cap"]))
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
