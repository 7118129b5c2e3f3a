"""GPU: match_tiles_split_kernel (gp_match.hip), the product's default matcher, against float64 at every live-block layout.

The inputs are hand-built f16 planes (gigapose_testing/stage_refs.py: match_blocks_case) whose 9 x 9 tiles hold every pair of
(live query-patch blocks, live template-patch blocks) in 0..8 x 0..8 -- all 81 entries of kMatchRect -- with patch 0 and patch 255 live
and dead in turn, fractional masks, bit-identical copies on both sides (exact ties across 32-row blocks) and the ragged last band of
8 + 1 crops.  match_tiles_f64 restates the reference matcher in float64 on the values the kernel reads; match_tiles_check accepts a
difference only where it sits on a float64 decision margin below eps = 2 c mag, c = 2 x the error of torch's own f32 evaluation of the
same products (never taken from the kernel), and never on an exact tie.  tests/test_stage_refs.py holds the CPU side: the cases'
preconditions, and seven subtly wrong matchers the checker rejects.

Every case asserts: no failed entry, excused entries <= 0.5 % of the checked ones, a clean status word, outputs fully overwritten
(pre-filled with NaN / 0xEE).  Hook-free cases run on both libraries (also_on_probe_binary); the uncompacted route of the compacted
masks needs the probe build's switch."""
import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from test_gpu_split import also_on_probe_binary, binary_name

pytestmark = pytest.mark.gpu
DEV = "cuda"


def launch(case, numerics="split"):
    """One launch of the tile matcher through LocalSimilarity.match_tiles on the case's planes (split) or its unit f32 features (chain),
    into pre-filled outputs -> dict of numpy arrays."""
    from gigapose_amd.matching import LocalSimilarity, MatchBank

    B, N, O, C = case["B"], case["N"], case["O"], case["C"]
    metric = LocalSimilarity(k=5, sim_threshold=case["thr"], patch_threshold=case["patch_thr"], search_direction=case["direction"])
    metric.numerics = numerics
    bank = MatchBank.__new__(MatchBank)
    bank.numerics, bank.bank_dtype, bank.O, bank.N, bank.C = numerics, "f32", O, N, C
    bank.features = bank.hi = bank.lo = None
    if numerics == "split":
        bank.hi = case["b_hi"].to(DEV).contiguous()
        bank.lo = None if case["b_lo"] is None else case["b_lo"].to(DEV).contiguous()
        query = (case["q_hi"].to(DEV).contiguous(), case["q_lo"].to(DEV).contiguous())
    else:
        bank.features = torch.from_numpy(case["t"]).to(DEV).transpose(2, 3).contiguous()           # (O, N, C, 256)
        query = torch.from_numpy(case["q"]).to(DEV).transpose(1, 2).contiguous()                   # (B, C, 256)
    bank.masks = torch.from_numpy(case["tm"]).to(DEV)
    out = (torch.full((B, N, 256), 0xEE, dtype=torch.uint8, device=DEV), torch.full((B, N, 256), float("nan"), device=DEV),
           torch.full((B, N, 256), float("nan"), device=DEV), torch.full((B, N), float("nan"), device=DEV))
    _lib.status_word(DEV).zero_()
    got = metric.match_tiles(query, torch.from_numpy(case["qm"]).to(DEV), bank, torch.from_numpy(case["labels"]).to(DEV).int(), out=out)
    torch.cuda.synchronize()
    assert _lib.take_status() == 0
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    res = {k: t.cpu().numpy() for k, t in zip(("idx", "score", "mask", "sim_avg"), out)}
    assert not any(np.isnan(res[k]).any() for k in ("score", "mask", "sim_avg")), "an output entry was not written"
    return res


def check(name, ours, ref, c, label=None):
    rep = sr.match_tiles_check(ours, ref, c)
    print(f"[{binary_name()}] {label or name}: checked {rep['checked']} excused {rep['excused']} failed {rep['failed']}; c {c:.3g}; "
          f"max score err / bound {rep['max_ratio']:.3f}; valid {int((ours['mask'] != 0).sum())} (float64 {int((ref['mask'] != 0).sum())})")
    assert rep["failed"] == 0, rep["first"]
    assert rep["excused"] <= sr.MATCH_EXCUSED_CAP * rep["checked"], rep
    return rep


@also_on_probe_binary
@pytest.mark.parametrize("name", list(sr.MATCH_CASES))
def test_split_matcher_vs_float64(name):
    """blocks_a / blocks_b at C = 64 (two k-steps), blocks_a at C = 1024, 32 (a single k-step) and 96; src2tar; no cycle check;
    sim_threshold 0.0 (the last value that still compacts) and -0.25 (the uncompacted route, live negatives); the one-plane bank
    (float64 on b_hi alone); three objects with distinct banks."""
    case, ref, c = sr.match_case(name)
    check(name, launch(case), ref, c)


@pytest.mark.probes     # gp_match_split_set_compact: an A/B switch of the probe build
def test_uncompacted_route_vs_float64():
    """The full 256 x 256 tile on blocks_a's masks -- the yardstick of the compaction test -- held to float64 itself."""
    case, ref, c = sr.match_case("blocks_a")
    lib = _lib.lib()
    try:
        lib.gp_match_split_set_compact(0)
        ours = launch(case)
    finally:
        lib.gp_match_split_set_compact(1)
    check("blocks_a", ours, ref, c, "blocks_a uncompacted")


@also_on_probe_binary
def test_chain_matcher_vs_float64():
    """gp_match_tiles_dir (the f32 fmaf chain, the oracle's twin) on blocks_a's unit f32 features, float64 on those features: the
    verification mode's decisions are tied to float64 at these layouts too."""
    case, _, _ = sr.match_case("blocks_a")
    q, t = torch.from_numpy(case["q"]), torch.from_numpy(case["t"])
    ref = sr.match_tiles_f64(q, None, t, None, case["qm"], case["tm"], case["labels"], case["thr"], case["patch_thr"], case["direction"], scale=1.0)
    c = sr.match_value_coeff(q, None, t, None, case["labels"], scale=1.0)
    check("blocks_a", launch(case, "chain"), ref, c, "blocks_a chain kernel")
