"""GPU: the IST regressor in split numerics (gp_ist_regress with the 20-pointer weight table) -- the compacted-row path itself.

gp_ist.hip compacts the live rows on the device (ist_gather_kernel: ballot + one atomic add per (b, j) block), runs the hidden layers
over the worst-case row count with tiles beyond the device row counter returning at once (gp_gemm_split_launch_limited) and maps rows
back in ist_head_kernel.  The stage tests of tests/test_gpu_pose_ist.py run the 12-pointer (chain) table; only eval_retrieval reached the
split one.  Here, through ISTNet.regress_bank with head_numerics = "split" (D = H = 256, O = 2, N = 5, B = 4, k = 3: R = 3072 rows = 24 column
tiles of 128), correspondence sets whose live-row count is exactly 0, 1 (in the last block), 127, 128, 129, 1280, 1281, R - 1 and R, plus
half-specified points:
  * invalid rows exactly -1000, valid rows finite;
  * valid rows against the float64 regressor on the gathered float64 features: max error <= 1.5 x and rms <= 1.25 x the error of the CPU
    oracle (oracle.cpu.ist_inference, the f32 fmaf chain the chain kernels are pinned to), + 1e-7 absolute for tanhf -- the project's
    criterion for split numerics (test_split_gemm_error_vs_f64_not_above_the_chain);
  * a live row's result does not depend on its compact position: bit-identical across the sets and across two runs of one call;
  * a workspace that served a call with more live rows gives the same bits as a fresh one;
  * the chain table on the same sets, bit-exact against the oracle;  status word 0 throughout."""
import numpy as np
import pytest
import torch

from gigapose_amd import _lib
from gigapose_testing import stage_refs as sr
from oracle import cpu as oracle
from test_oracle_pose_ist import build_ist, mlp_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
O, N, B, K = 2, 5, 4, 3
R = B * K * sr.P


@pytest.fixture(autouse=True)
def clean_status():
    _lib.status_word(DEV).zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_word(DEV).zero_()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    def __init__(self, numerics, seed=111):
        self.net = build_ist(seed)
        self.w = mlp_weights(self.net)
        self.seed = seed
        self.numerics = numerics
        rs = np.random.RandomState(seed + 1)
        self.bank = rs.standard_normal((O, N, 256, 16, 16)).astype(np.float32)
        self.tar = rs.standard_normal((B, 256, 16, 16)).astype(np.float32)
        self.labels0 = rs.randint(0, O, B).astype(np.int32)
        self.ids = rs.randint(0, N, (B, K)).astype(np.int64)
        self.points = sr.ist_points_case(seed + 2, B, K)
        self.dev = (t(self.bank), t(self.labels0), t(self.ids), t(self.tar))
        self.module = self.fresh_module()

    def fresh_module(self):
        net = build_ist(self.seed).to(DEV)
        net.head_numerics = self.numerics
        return net

    def run(self, tp, sp, module=None):
        net = module or self.module
        sc, cs = net.regress_bank(self.dev[0], self.dev[1], self.dev[2], self.dev[3], t(sp), t(tp))
        torch.cuda.synchronize()
        assert len(net._packed[1]) == (20 if self.numerics == "split" else 12)      # the weight table the launch took
        _lib.check_status()
        return sc.cpu().numpy().reshape(R), cs.cpu().numpy().reshape(R, 2)

    def oracle(self, tp, sp):
        osc, ocs = oracle.ist_inference(self.tar.reshape(B, 256, 256), self.bank.reshape(O, N, 256, 256)[self.labels0[:, None], self.ids], tp, sp, self.w)
        return osc.reshape(R), ocs.reshape(R, 2)

    def f64(self, tp, sp, rows):
        sc, cs = sr.ist_regressor_f64(sr.ist_gather_f64(self.tar, self.bank, self.labels0, self.ids, tp, sp, rows), self.w)
        return sc.numpy(), cs.numpy()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_validity(sc, cs, live):
    assert (sc[~live] == -1000.0).all() and (cs[~live] == -1000.0).all(), "an invalid row is not exactly -1000"
    assert np.isfinite(sc[live]).all() and np.isfinite(cs[live]).all() and (sc[live] != -1000.0).all() and (np.abs(cs[live]) <= 1.0).all()


def test_ist_split_live_row_counts_vs_float64_and_row_independence():
    case = Case("split")
    tar, src, order = case.points
    results = {}
    for n in sr.IST_LIVE_COUNTS:
        tp, sp, live = sr.ist_live_set(tar, src, order, n)
        sc, cs = case.run(tp, sp)
        check_validity(sc, cs, live)
        if n == 0:
            assert (sc == -1000.0).all() and (cs == -1000.0).all()
        sc2, cs2 = case.run(tp, sp)                                            # run to run: the atomics hand out rows in any order
        assert (u32(sc) == u32(sc2)).all() and (u32(cs) == u32(cs2)).all(), f"{n} live rows: two runs of one call differ"
        results[n] = (sc, cs, live)
        if n == 0:
            continue
        rows = np.nonzero(live)[0]
        rsc, rcs = case.f64(tp, sp, rows)
        osc, ocs = case.oracle(tp, sp)
        assert ((osc == -1000.0) == ~live).all()
        for name, got, orc, ref, tanh_abs in (("scale", sc[rows], osc[rows], rsc, 0.0), ("cos_sin", cs[rows], ocs[rows], rcs, 1e-7)):
            e_s, e_o = np.abs(got - ref), np.abs(orc - ref)
            rms = lambda e: float(np.sqrt((e ** 2).mean()))
            print(f"IST split, {n:4d} live rows, {name:7s}: max err vs f64 split {e_s.max():.3e} oracle {e_o.max():.3e} (ratio "
                  f"{e_s.max() / e_o.max() if e_o.max() else float('nan'):.2f}); rms split {rms(e_s):.3e} oracle {rms(e_o):.3e} (ratio "
                  f"{rms(e_s) / rms(e_o) if rms(e_o) else float('nan'):.2f}); max |ref| {np.abs(ref).max():.2f}")
            assert e_s.max() <= 1.5 * e_o.max() + tanh_abs, (n, name, e_s.max(), e_o.max())
            assert rms(e_s) <= 1.25 * rms(e_o) + tanh_abs, (n, name, rms(e_s), rms(e_o))
    # row independence: the sets are nested, a row live in two of them has the same points and another compact position
    full_sc, full_cs, _ = results[R]
    for n, (sc, cs, live) in results.items():
        assert (u32(sc[live]) == u32(full_sc[live])).all() and (u32(cs[live]) == u32(full_cs[live])).all(), \
            f"rows of the {n}-live set differ from the same rows of the all-live set"


def test_ist_split_half_specified_points_are_invalid():
    case = Case("split")
    tar, src, order = case.points
    tp, sp, live = sr.ist_live_set(tar, src, order, 1280)
    base_sc, base_cs = case.run(tp, sp)
    tp2, sp2, rows = sr.ist_half_specified(tp, sp, live, 9)
    sc, cs = case.run(tp2, sp2)
    check_validity(sc, cs, live)
    assert (sc[rows] == -1000.0).all() and (cs[rows] == -1000.0).all()
    assert (u32(sc) == u32(base_sc)).all() and (u32(cs) == u32(base_cs)).all()      # the live rows are untouched by their new neighbours
    osc, ocs = case.oracle(tp2, sp2)
    assert ((osc == -1000.0) == (sc == -1000.0)).all()


def test_ist_split_workspace_reuse_equals_fresh_modules():
    """R live, then 1 live, then 0 live on the SAME module (the hidden-layer buffers still hold the larger call's columns; the last
    128-column tile of the 1-live call is 127 stale columns wide) == each call on a fresh module, bit for bit."""
    case = Case("split")
    tar, src, order = case.points
    for n in (R, 1, 0):
        tp, sp, live = sr.ist_live_set(tar, src, order, n)
        sc, cs = case.run(tp, sp)
        fsc, fcs = case.run(tp, sp, case.fresh_module())
        check_validity(sc, cs, live)
        assert (u32(sc) == u32(fsc)).all() and (u32(cs) == u32(fcs)).all(), f"{n} live rows after a larger call differ from a fresh workspace"


def test_ist_chain_table_on_the_same_sets_vs_oracle():
    """The 12-pointer table at the same edges: the scale head (no transcendental) bit-exact against the oracle's fmaf chains, cos / sin to
    tanhf's device-vs-glibc difference -- as test_ist_regressor_vs_oracle_and_golden asserts for its one set."""
    case = Case("chain")
    tar, src, order = case.points
    sets = [sr.ist_live_set(tar, src, order, n) for n in sr.IST_LIVE_COUNTS]
    tp, sp, live = sr.ist_live_set(tar, src, order, 1280)
    tp2, sp2, _ = sr.ist_half_specified(tp, sp, live, 9)
    sets.append((tp2, sp2, live))
    for tp, sp, live in sets:
        sc, cs = case.run(tp, sp)
        check_validity(sc, cs, live)
        osc, ocs = case.oracle(tp, sp)
        np.testing.assert_array_equal(u32(sc), u32(osc))
        np.testing.assert_allclose(cs, ocs, rtol=0, atol=5e-7)
        assert ((ocs == -1000.0) == (cs == -1000.0)).all()
