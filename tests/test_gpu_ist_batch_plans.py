"""GPU: the IST ResNet in split numerics under EVERY launch plan a batch size selects.

conv_planes_kernel, conv_halo_kernel and the stem build (gp_conv256.hip) run no fixed schedule: the host picks a plan from the tile count
-- batch size x a constant of the layer -- and GpSlotPlan cuts each XCD's chunk of tiles into data-parallel rounds, whole tiles, published
heads, received rests and middle segments.  gigapose_testing/conv_plans.py calls those decisions (gp_plan256.h); tests/test_conv_plans.py enumerates
the 78 plan classes of B = 1 .. 64 (20 of them reached at B = 1, 3, 5, where the backbone was compared with float64 until now) and holds
conv_plans.BATCHES to running every one.  Here, for each B of that list, on the product binary:

* split numerics against oracle.ist_torch.resnet_forward in float64 under the project's criterion for this backbone, unchanged
  (test_ist_backbone_split_vs_chain_and_torch): max error < 2e-5 of max |feature| and <= 1.5 x the chain mode's error on the same batch + 1e-7;
* chain numerics: every row bit-identical to the chain result of its crop run alone (the chain mode's batch invariance);
* split numerics twice: bit-identical (the hand-over order is fixed by the shape); everything finite, the status word clean;
* ONE module across the whole sweep, ascending then descending (its ping-pong buffers and stem planes only grow, the scratch keeps old
  epochs): every result equals a fresh module's, bit for bit;
* ISTNet.forward_by_chunk at 65 and 127 crops == the backbone on the chunks 64 + 1 and 64 + 63.

Row r of a batch of B is pool crop (r + B) % 6, so one crop lands in different rows, tiles and XCD chunks from batch to batch and its
float64 features are computed once.  Every buffer a forward allocates uninitialised (torch.empty: the output, the ping-pong buffers,
the stem planes) is pre-filled with NaN: what a plan leaves unwritten shows.

test_trace_ties_the_host_model_to_the_kernels (probe build) is what makes the model an authority: per slot, the segments and k-steps the
kernels count equal the model's for every entry of conv_plans.STAGE_SHAPES."""
import contextlib
import copy
import ctypes
from unittest import mock

import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import conv_plans
from gigapose_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCHES = [B for B, _ in conv_plans.BATCHES]
NPOOL = 6


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


@contextlib.contextmanager
def nan_filled_allocations():
    """torch.empty hands out NaN for the duration: the output, ping-pong buffers and stem planes of ResNet.forward."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    with mock.patch.object(torch, "empty", empty):
        yield


def bits(t):
    return t.contiguous().view(torch.int32)


def rows(n):
    """Pool indices of the rows of a batch of n crops."""
    return [(r + n) % NPOOL for r in range(n)]


class Sweep:
    """The pool, its float64 features, a module factory and the per-B results shared by the tests of this module (computed once)."""

    def __init__(self):
        from oracle import ist_torch
        from test_oracle_pose_ist import build_ist

        net = build_ist(101)
        tmpl, _ = syn.template_images(102, 2)
        # the pool of test_resnet_split_other_batch_sizes_vs_chain_and_torch (5 crops) and a sixth in its manner
        pool = np.concatenate([tmpl, tmpl[:1] * 0.5, tmpl[::-1] * 0.8, tmpl[1:] * 1.3])
        assert pool.shape[0] == NPOOL and len({p.tobytes() for p in pool}) == NPOOL
        self.pool_cpu = torch.from_numpy(np.ascontiguousarray(pool))
        with torch.no_grad():
            self.ref = ist_torch.resnet_forward(net.backbone.double(), self.pool_cpu.double()).numpy()      # (6, 256, 16, 16) float64, once
        self.net = net.float().to(DEV)           # never run: the template every fresh module is copied from
        self.pool = self.pool_cpu.to(DEV)
        self.results = {}
        with nan_filled_allocations():
            one = self.fresh("chain")
            self.chain_alone = [one(self.pool[i:i + 1]).clone() for i in range(NPOOL)]
        torch.cuda.synchronize()
        _lib.check_status()

    def fresh(self, numerics):
        """A ResNet that has run nothing: no buffers, no scratch, no packed weights."""
        return copy.deepcopy(self.net.backbone).set_numerics(numerics)

    def batch(self, n):
        return self.pool[torch.tensor(rows(n), device=DEV)].contiguous()

    def at(self, B):
        """-> (split on a fresh module, the same module again, chain on a fresh module) for the batch of B, cached."""
        if B not in self.results:
            x = self.batch(B)
            with nan_filled_allocations():
                m = self.fresh("split")
                s1 = m(x).clone()
                s2 = m(x).clone()
                ch = self.fresh("chain")(x).clone()
            torch.cuda.synchronize()
            _lib.check_status()
            self.results[B] = (s1, s2, ch)
        return self.results[B]

    def errors(self, n, split, chain):
        """The project's criterion on a batch: (split error, chain error) relative to max |feature| of the batch, and per row the split error
        relative to max |feature| of that row's crop."""
        ref = self.ref[rows(n)]
        scale = np.abs(ref).max()
        e_split, e_chain = (np.abs(v.cpu().numpy().astype(np.float64) - ref).max() / scale for v in (split, chain))
        d = np.abs(split.cpu().numpy().astype(np.float64) - ref).reshape(n, -1).max(axis=1)
        return e_split, e_chain, d / np.abs(ref).reshape(n, -1).max(axis=1)


@pytest.fixture(scope="module")
def sweep():
    return Sweep()


def test_batch_list_is_the_models():
    assert BATCHES == sorted(BATCHES) and BATCHES[-1] == 64 and sum(BATCHES) < 600


@pytest.mark.parametrize("B", BATCHES)
def test_ist_backbone_at_every_plan_vs_float64_and_chain(sweep, B):
    split, again, chain = sweep.at(B)
    assert split.shape == (B, 256, 16, 16)
    assert bool(torch.isfinite(split).all()) and bool(torch.isfinite(chain).all())
    assert torch.equal(bits(split), bits(again)), "two split forwards of one batch differ"
    for r, i in enumerate(rows(B)):      # chain: batch-invariant, bit for bit
        assert torch.equal(bits(chain[r]), bits(sweep.chain_alone[i][0])), f"chain row {r} (crop {i}) differs from the crop run alone"
    e_split, e_chain, e_rows = sweep.errors(B, split, chain)
    print(f"IST backbone B={B:2d} vs f64 torch: chain {e_chain:.2e}, split {e_split:.2e} (relative to max |feature|); worst row {int(e_rows.argmax())}: "
          f"{e_rows.max():.2e} of its own max |feature|")
    assert e_split < 2e-5 and e_split <= 1.5 * e_chain + 1e-7
    assert (e_rows < 2e-5).all(), e_rows      # every row against its crop's features, as a batch of its own would be held


def test_one_module_across_the_sweep_equals_fresh_modules(sweep):
    """Ascending, then descending: after a larger batch the plane halves of the ping-pong buffers sit at other offsets, _framed is
    re-allocated per B, the scratch holds the fragments and epochs of every launch before."""
    fresh = {B: sweep.at(B)[0] for B in BATCHES}
    one = sweep.fresh("split")
    for B in BATCHES + BATCHES[::-1]:
        got = one(sweep.batch(B))
        assert torch.equal(bits(got), bits(fresh[B])), f"B = {B} on the module of the sweep differs from a fresh module"
    torch.cuda.synchronize()
    _lib.check_status()


@pytest.mark.parametrize("n", [65, 127])
def test_forward_by_chunk_is_the_backbone_on_the_chunks(sweep, n):
    """max_batch_size = 64: 64 + 1 and 64 + 63 crops."""
    x = sweep.batch(n)
    outs = {}
    with nan_filled_allocations():
        for numerics in ("split", "chain"):
            net = copy.deepcopy(sweep.net)
            assert net.max_batch_size == 64
            net.backbone.set_numerics(numerics)
            outs[numerics] = net.forward_by_chunk(x).clone()
        parts = torch.cat([sweep.fresh("split")(x[:64]), sweep.fresh("split")(x[64:])], dim=0)
    torch.cuda.synchronize()
    _lib.check_status()
    assert outs["split"].shape == (n, 256, 16, 16) and bool(torch.isfinite(outs["split"]).all())
    assert torch.equal(bits(outs["split"]), bits(parts))
    e_split, e_chain, e_rows = sweep.errors(n, outs["split"], outs["chain"])
    print(f"forward_by_chunk {n} crops vs f64 torch: chain {e_chain:.2e}, split {e_split:.2e}; worst row {e_rows.max():.2e} of its own max |feature|")
    assert e_split < 2e-5 and e_split <= 1.5 * e_chain + 1e-7 and (e_rows < 2e-5).all()


def test_largest_errors_of_the_sweep(sweep):
    """The figures the sweep is summarised by (printed; every B is asserted above)."""
    es = {B: sweep.errors(B, sweep.at(B)[0], sweep.at(B)[2])[:2] for B in BATCHES}
    bs, bc = max(es, key=lambda B: es[B][0]), max(es, key=lambda B: es[B][1])
    print(f"largest split error {es[bs][0]:.2e} at B = {bs}; largest chain error {es[bc][1]:.2e} at B = {bc}")
    assert all(e[0] < 2e-5 for e in es.values())


# ---------------------------------------------------------------------------------------------------------------- model <-> kernels
def planes(t, scale):
    t = t.contiguous()
    hi = torch.empty(t.shape, dtype=torch.float16, device=t.device)
    lo = torch.empty_like(hi)
    _lib.call("gp_split_planes", _lib.ptr(t), ctypes.c_size_t(t.numel()), _lib.f(scale), _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr())
    return hi, lo


@pytest.mark.probes     # gp_conv2d_planes_set_trace: the traced build
def test_trace_ties_the_host_model_to_the_kernels():
    """Words 0 and 1 of a slot's 8 trace words: segments run, k-steps run (the halo kernel counts 9 per channel block).  For every entry of
    STAGE_SHAPES they equal the model's per-slot segment count and unit total; slots beyond the grid write nothing.  Then the stem build
    at one batch size of each of its six classes."""
    lib = _lib.lib()
    nb = lib.gp_conv2d_planes_workspace_bytes()
    ws = torch.zeros(nb // 4, device=DEV)
    trace = torch.zeros(256, 8, dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(5)
    try:
        for (cin, cout, k, stride, pad, hw, B, res), _, why in conv_plans.STAGE_SHAPES:
            plan = conv_plans.launch_slots(conv_plans.conv_launch(B, hw, hw, cin, cout, k, k, stride, pad))
            oh = (hw + 2 * pad - k) // stride + 1
            xh, xl = planes(torch.randn(B, hw, hw, cin, generator=g).to(DEV), 8.0)
            wh, wl = planes((torch.randn(cout, k * k * cin, generator=g) / np.sqrt(k * k * cin)).to(DEV), 64.0)
            rh, rl = planes(torch.randn(B, oh, oh, cout, generator=g).to(DEV), 8.0) if res else (None, None)
            al, be = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
            ohi, olo = (torch.zeros(B, oh, oh, cout, dtype=torch.float16, device=DEV) for _ in range(2))
            trace.zero_()
            lib.gp_conv2d_planes_set_trace(ctypes.c_void_p(trace.data_ptr()))
            _lib.call("gp_conv2d_planes", _lib.ptr(xh), _lib.ptr(xl), _lib.ptr(wh), _lib.ptr(wl), _lib.ptr(al), _lib.ptr(be), _lib.ptr(rh), _lib.ptr(rl),
                      _lib.i(B), _lib.i(hw), _lib.i(hw), _lib.i(cin), _lib.i(cout), _lib.i(k), _lib.i(k), _lib.i(stride), _lib.i(pad), _lib.i(1),
                      _lib.ptr(ohi), _lib.ptr(olo), _lib.ptr(None), _lib.ptr(ws), ctypes.c_size_t(nb), _lib.stream_ptr())
            torch.cuda.synchronize()
            lib.gp_conv2d_planes_set_trace(None)
            _lib.check_status()
            got = trace.cpu().numpy()
            want = np.zeros((256, 2), np.int64)
            for p, w in conv_plans.trace_words(plan).items():
                want[p] = w
            bad = np.nonzero((got[:, :2] != want).any(axis=1))[0]
            print(f"trace {why}: grid {plan['grid']}, {int(want[:, 0].sum())} segments, {int(want[:, 1].sum())} k-steps; slots that differ: {bad.tolist()}")
            assert bad.size == 0, (why, [(int(p), got[p, :2].tolist(), want[p].tolist()) for p in bad[:8]])
            assert not got[plan["grid"]:].any()
        # the stem build (gp_conv2d_stem_planes, 7 k-steps per tile) at a batch size of each of its six classes; the values play no part
        S, cout = 256, 128
        wz = torch.zeros(cout, 224, dtype=torch.float16, device=DEV)
        seen = set()
        for B in (1, 2, 4, 5, 8, 9):
            plan = conv_plans.launch_slots(conv_plans.stem_launch(B, S, cout))
            seen.add(conv_plans.plan_class(plan))
            fz = torch.zeros(B, S + 6, S + 8, 4, dtype=torch.float16, device=DEV)
            ohi, olo = (torch.zeros(B * (S // 2) ** 2, cout, dtype=torch.float16, device=DEV) for _ in range(2))
            trace.zero_()
            lib.gp_conv2d_planes_set_trace(ctypes.c_void_p(trace.data_ptr()))
            _lib.call("gp_conv2d_stem_planes", _lib.ptr(fz), _lib.ptr(fz), _lib.ptr(wz), _lib.ptr(wz), _lib.ptr(None), _lib.ptr(None), _lib.i(B), _lib.i(S),
                      _lib.i(cout), _lib.i(1), _lib.ptr(ohi), _lib.ptr(olo), _lib.ptr(ws), ctypes.c_size_t(nb), _lib.stream_ptr())
            torch.cuda.synchronize()
            lib.gp_conv2d_planes_set_trace(None)
            _lib.check_status()
            got = trace.cpu().numpy()
            want = np.array([conv_plans.trace_words(plan)[p] for p in range(256)], np.int64)
            bad = np.nonzero((got[:, :2] != want).any(axis=1))[0]
            print(f"trace stem B={B}: {conv_plans.describe_class(conv_plans.plan_class(plan))}; slots that differ: {bad.tolist()}")
            assert bad.size == 0, (B, [(int(p), got[p, :2].tolist(), want[p].tolist()) for p in bad[:8]])
        assert len(seen) == 6
    finally:
        lib.gp_conv2d_planes_set_trace(None)
