"""CPU: the IST convolutions' launch plans (gigapose_testing/conv_plans.py calls gp_plan256.h's gp_conv256_plan, gp_stem256_plan and
GpSlotPlan -- the code gp_conv2d_planes, gp_conv2d_stem_planes and their kernels run, compiled for the host) checked exhaustively --
every layer of IST_CFG at every batch size from 1 to 64 and at 65, 96, 127, 128:

* every (tile, unit) is computed exactly once;
* serial plans: a rest or middle segment continues exactly where slot p - 8 stopped, a chain starts at unit 0 and ends at the tile's last
  unit in the one slot that runs the epilogue;
* parallel split: the parts of a tile are disjoint and cover it, the owner holds the last part, and the flags gp_handoff_wait is given are
  exactly those of the other parts;
* the plan classes over B = 1 .. 64 are enumerated and printed, and the case lists of the GPU tests are held to them: BATCHES runs every
  class, STAGE_SHAPES has every property of every class of gp_conv2d_planes and the plans it promises.

That the kernels run what the plan says is the trace test's business (tests/test_gpu_ist_batch_plans.py: segments and k-steps per slot)."""
import functools

import pytest

from gigapose_testing import conv_plans as cp
from test_oracle_pose_ist import IST_CFG

SIZES = list(range(1, 65)) + [65, 96, 127, 128]


def test_model_configuration_is_the_suites():
    assert cp.IST_CFG == IST_CFG


def launch_key(launch):
    return tuple(sorted(launch.items()))


@functools.lru_cache(maxsize=None)
def distinct_launches():
    """Every distinct launch (kernel, tiles, units per tile, plan) over SIZES -> {key: (launch, first (B, layer))}; 21 launches per forward."""
    out = {}
    for B in SIZES:
        launches = cp.ist_layer_launches(IST_CFG, B)
        assert len(launches) == 21 and launches[0][0] == "stem" and all(l is not None for _, l in launches)
        for name, launch in launches:
            out.setdefault(launch_key(launch), (launch, (B, name)))
    return out


def check_plan(plan, where):
    upt, par = plan["upt"], plan["par"]
    pieces = {}                                   # tile -> [(u0, u1, p, kind)]
    for p, segs in plan["slots"].items():
        kinds = [k for *_, k in segs]
        # order inside a slot: data-parallel rounds, the published head (or middle), whole tiles, the received rest
        rank = {"dp": 0, "head": 1, "middle": 1, "whole": 2, "rest": 3}
        assert kinds == sorted(kinds, key=rank.get), (where, p, kinds)
        assert sum(k in ("head", "middle") for k in kinds) <= 1 and sum(k in ("rest", "middle") for k in kinds) <= 1, (where, p, kinds)
        if "middle" in kinds:                     # it is the slot's only segment outside the data-parallel rounds
            assert [k for k in kinds if k != "dp"] == ["middle"], (where, p, kinds)
        for tile, u0, u1, kind in segs:
            assert 0 <= tile < plan["tiles"] and 0 <= u0 < u1 <= upt, (where, p, tile, u0, u1)
            assert (u0 == 0) == (kind in ("dp", "head", "whole")) and (u1 == upt) == (kind in ("dp", "whole", "rest")), (where, p, tile, u0, u1, kind)
            pieces.setdefault(tile, []).append((u0, u1, p, kind))
    assert sorted(pieces) == list(range(plan["tiles"])), where
    for tile, ps in pieces.items():               # every (tile, unit) exactly once: the pieces are disjoint and cover [0, upt)
        ps.sort()
        assert ps[0][0] == 0 and ps[-1][1] == upt and all(a[1] == b[0] for a, b in zip(ps, ps[1:])), (where, tile, ps)
        # one slot runs the epilogue, and it holds the tile's last unit; every other piece is published
        assert [k in ("dp", "whole", "rest") for *_, k in ps] == [False] * (len(ps) - 1) + [True], (where, tile, ps)
        slots = [p for _, _, p, _ in ps]
        assert all(b == a + 8 for a, b in zip(slots, slots[1:])), (where, tile, slots)          # neighbouring slots of ONE XCD, in k order
        owner = slots[-1]
        if par:
            S = plan["par_S"][owner & 7]
            assert len(ps) == S and [(u0, u1) for u0, u1, _, _ in ps] == [(upt * i // S, upt * (i + 1) // S) for i in range(S)], (where, tile, ps)
            # x + 8 (n - 1) down to x + 8 m_lo: exactly the flags of the other parts, nearest first
            assert cp.handoff_wait_flags(plan, owner) == slots[-2::-1], (where, tile, slots)
            assert all(cp.handoff_wait_flags(plan, q) == [] for q in slots[:-1])
        else:
            for (u0, u1, q, kind), prev in zip(ps[1:], ps):   # continues where slot q - 8 stopped, and waits for that slot's flag only
                assert kind in ("rest", "middle") and cp.handoff_wait_flags(plan, q) == [q - 8] == [prev[2]] and prev[3] in ("head", "middle") and prev[1] == u0
    if par:
        assert all(len(s) <= 1 for s in plan["slots"].values()) and set(plan["par_S"]) == set(range(8))
    words = cp.trace_words(plan)
    assert sum(w[1] for w in words.values()) == plan["tiles"] * upt * plan["steps_per_unit"]


def test_every_plan_computes_every_unit_once_and_pairs_its_hand_overs():
    n_middle = 0
    for launch, where in distinct_launches().values():
        plan = cp.launch_slots(launch)
        check_plan(plan, where)
        kinds = {k for s in plan["slots"].values() for *_, k in s}
        n_middle += "middle" in kinds
    print(f"{len(distinct_launches())} distinct launches over B = {SIZES[0]} .. {SIZES[-1]}, {n_middle} with a middle segment")
    assert n_middle > 0


def test_the_middle_segment_of_layer3_conv1_at_ten_crops():
    """The case the model was written for: 192 -> 256, 3 x 3 / stride 2 from 64 x 64 at B = 10 is 40 tiles of 54 k-steps on 64 slots; slot 2 of
    every XCD gets units 67 .. 100 of its chunk of 5 tiles -- k-steps 13 .. 46 of the chunk's second tile, neither its first nor its last."""
    launch = dict(cp.ist_layer_launches(IST_CFG, 10))["layer3.0.conv1"]
    assert (launch["kernel"], launch["tiles"], launch["upt"], launch["slots_x"], launch["par"]) == ("gather", 40, 54, 8, False)
    plan = cp.launch_slots(launch)
    for x in range(8):
        assert plan["slots"][x + 8 * 2] == [(5 * x + 1, 13, 47, "middle")]
        assert plan["slots"][x + 8 * 1][0][:3] == (5 * x + 1, 0, 13) and plan["slots"][x + 8 * 3][-1][:3] == (5 * x + 1, 47, 54)


@functools.lru_cache(maxsize=None)
def classes_by_batch():
    return {B: cp.ist_classes(IST_CFG, B) for B in range(1, 65)}


def test_plan_classes_are_enumerated_and_the_batch_list_runs_every_one():
    per_b = classes_by_batch()
    every = {}
    for B, cs in per_b.items():
        for c, layer in cs.items():
            every.setdefault(c, []).append(B)
    old = set(per_b[1]) | set(per_b[3]) | set(per_b[5])
    print(f"{len(every)} plan classes over B = 1 .. 64, {len(set(every) - old)} of them not reached at B = 1, 3, 5:")
    for c in sorted(every):
        bs = every[c]
        print(f"  {cp.describe_class(c):100s} {'' if c in old else 'new '} B = {', '.join(map(str, bs[:8]))}{', ..' if len(bs) > 8 else ''}")
    assert len(every) == 78 and len(old) == 20     # a change of the launchers or of GpSlotPlan changes the enumeration: revisit both lists
    names = {cp.describe_class(c): c for c in every}
    assert len(names) == len(every)
    batches = [B for B, _ in cp.BATCHES]
    assert batches == sorted(set(batches)) and 1 <= batches[0] and batches[-1] == 64
    named, run = set(), set()
    for B, there_for in cp.BATCHES:
        run |= set(per_b[B])
        for name in there_for:
            assert name in names and names[name] in per_b[B], (B, name)     # the class an entry is there for is a class of that batch size
            assert name not in named, name
            named.add(name)
        print(f"  B = {B:2d} runs {len(per_b[B]):2d} classes, is there for {len(there_for)}")
    assert not set(every) - run, [cp.describe_class(c) for c in set(every) - run]      # no class is left out
    assert named == set(names)
    middle = [c for c in every if c[0] == "gather" and "middle" in c[4]]
    assert middle and not any(c in old for c in middle)                     # the gather kernel's middle segment: new to the suite


def test_stage_shapes_have_every_property_of_every_class_and_the_promised_plans():
    per_b = classes_by_batch()
    every = {c for cs in per_b.values() for c in cs if c[0] != "stem"}       # gp_conv2d_planes: the gather and the halo kernel
    assert len(cp.STAGE_SHAPES) <= 16 and len({s for s, _, _ in cp.STAGE_SHAPES}) == len(cp.STAGE_SHAPES)
    got, feats = {}, set()
    for shape, promised, why in cp.STAGE_SHAPES:
        launch = cp.stage_launch(shape)
        assert launch is not None, shape                                    # not refused by the entry point
        plan = cp.launch_slots(launch)
        check_plan(plan, shape)
        c = cp.plan_class(plan)
        assert cp.describe_class(c) == promised, (shape, cp.describe_class(c))
        got[shape] = (c, launch)
        feats |= cp.class_features(c)
        print(f"  {str(shape):42s} {launch['tiles']:3d} tiles x {launch['upt']:3d}: {promised}  [{why}]{'' if c in every else '  (no IST layer has it)'}")
    want = set().union(*(cp.class_features(c) for c in every))
    assert not want - feats, sorted(want - feats, key=str)
    exact = {c for c, _ in got.values()} & every
    print(f"{len(want)} properties of {len(every)} classes, all in the list; {len(exact)} classes occur whole")

    def has(pred):
        return [s for s, (c, l) in got.items() if pred(s, c, l)]
    # (cin, cout, k, stride, pad, hw, B, res); class (kernel, mode, slots_x, div8, kinds, par_S, idle)
    assert has(lambda s, c, l: c[0] == "gather" and "middle" in c[4] and s[7])                                   # a gather middle segment, with a residual
    for sx in (2, 4, 8, 16):
        assert has(lambda s, c, l: c[0] == "gather" and c[2] == sx and "head" in c[4] and "rest" in c[4]), sx    # gather chains of hand-overs
    assert has(lambda s, c, l: c[:2] == ("halo", "serial") and "head" in c[4] and "dp" not in c[4])              # halo serial with cut tiles
    assert has(lambda s, c, l: c[:2] == ("halo", "serial") and "head" in c[4] and "dp" in c[4])                  # ... data-parallel rounds + a cut remainder
    assert has(lambda s, c, l: c[:2] == ("halo", "par") and len(c[5]) == 2)                                      # two par_S in one launch
    assert has(lambda s, c, l: c[:2] == ("halo", "par") and c[5] == (1,) and c[6])                               # S = 1 and idle slots
    assert has(lambda s, c, l: c[:2] == ("halo", "par") and s[1] == 64)                                          # parallel at Cout = 64
    for tiles in (7, 8, 255, 256, 257):
        assert has(lambda s, c, l: c[0] == "halo" and l["tiles"] == tiles), tiles
    assert has(lambda s, c, l: c[:2] == ("halo", "par") and s[7])                                                # a residual on a parallel case
    for s in got:                                                                                                # halo cases 16 x 16, gather 3 x 3 / 2 from 32 x 32 or 1 x 1
        assert (s[2:6] == (3, 1, 1, 16) and s[0] in (64, 128, 512)) or s[2:6] == (3, 2, 1, 32) or s[2:5] == (1, 1, 0), s


@pytest.mark.parametrize("shape,why", [((1, 24, 24, 128, 128, 3, 3, 1, 1), "576 pixels"), ((2, 16, 16, 48, 128, 1, 1, 1, 0), "Cin = 48"),
                                       ((2, 16, 16, 64, 96, 1, 1, 1, 0), "Cout = 96")])
def test_refused_sizes_have_no_plan(shape, why):
    assert cp.conv_launch(*shape) is None, why
