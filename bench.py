#!/usr/bin/env python
"""Headline benchmark: query-crops/sec through the whole coarse-pose hot path
(ViT feat + template NN + 4DoF regress; BASELINE.json metric) on MI355X.

A "step" = one pass of gigapose_amd.GigaPose.predict over one batch of B synthetic 224x224 crops
already resident in HBM, against an onboarded bank of O objects x 162 templates:
DINOv2 ViT-L/14 features -> fused template matching -> IST backbone + regressor -> RANSAC -> pose.
N=1 workload = BASELINE.json configs[1]: ViT-L/14 random-init, 1 object x 162 templates, B=64.
N>1 (one rank per GPU, torch.distributed / RCCL): weak scaling, B crops per rank, template bank
sharded by template index with the two all-gathers of gigapose_amd/sharding.py (configs[3] shape).

Prints ONE JSON line on rank 0.  A plain run (`bench.py --gpus N --steps K --warmup W`) sets up, warms up, times
the K steps and prints the headline (`value`, `ms_per_step`, `dtype`, `config`) -- nothing else.  `--full` adds
everything else this file measures: `roofline` (dominant kernel family timed by HIP events on the launch stream
inside the timed region, a per-family replay, the matrix-ceiling micro-benchmark), the other numerics modes, the
BASELINE config-3 / config-5 shapes and the batch curve, the drop-in flow, the other multi-GPU mode (N > 1) and
`cpu_baseline` (the CPU oracle port timed on the host cores on a bounded sample; N=1 only).
`--dump-outputs DIR` writes what the last timed step returned (see dump_outputs).
"""
import argparse
import ctypes
import json
import os
import sys
import time

# kernel arguments in device memory instead of host memory the command processor reads over the fabric: the step has ~210
# dependent launches, and each starts 1-2 us earlier (measured A/B on one box: 45.95 -> 45.65 ms per step).  A HIP runtime
# setting, read when the runtime is loaded -- hence before `import torch`; an exported value wins.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
# N > 1: the host driver of this pool supports dmabuf IPC only; without it RCCL's buffer registration across ranks fails with
# `hipIpcGetMemHandle: invalid argument`.  Exported on the GPU boxes already; kept here so that the line does not depend on the shell.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X dense f32-input MFMA peak (MI355X_MICROARCH.md)
FLOP_PER_CROP = {"dinov2_vitl14": 162.0e9, "dinov2_vits14": 12.25e9, "dinov2_vitb14": 0.0}
ANCHOR_FILE = os.path.join(ROOT, "profiles", "r06_cpu_reference_vs_port.txt")


DUMP_BYTES = 64 << 20   # --dump-outputs: at most this many bytes of .npy data in all


def host_outputs(pred):
    """The arrays a caller of GigaPose.predict receives (every tensor of the returned collection), on the host as float32 (floating
    tensors) or float64 (integer / bool tensors: exact for every index and count the path returns)."""
    out = {}
    for name, t in (pred.tensors.items() if pred is not None else ()):
        a = t.detach().cpu()
        if a.dtype != torch.float64:
            a = a.float() if a.is_floating_point() else a.to(torch.float64)
        out[name] = a.numpy()
    return out


def dump_outputs(outputs, out_dir):
    """DIR/<name>.npy per output array.  Should the arrays exceed DUMP_BYTES in all (large --batch / --k), every array is replaced by a
    fixed, seeded sample of its flattened elements (in index order), each array keeping its share of the budget."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in outputs.values())
    for name, a in sorted(outputs.items()):
        if total > DUMP_BYTES:
            n = max(1, a.size * DUMP_BYTES // total)
            a = a.reshape(-1)[np.sort(np.random.RandomState(0).choice(a.size, n, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def reference_over_port(threads):
    """unmodified reference / oracle.torch_port wall-clock ratio, same crops + threads + process, measured in the build container by
    oracle/time_reference.py at the thread count it is applied to: read from the committed measurement file."""
    vals = {}
    try:
        for ln in open(ANCHOR_FILE):
            if ln.startswith("reference_over_port_") and "=" in ln:
                k, v = ln.split("=")
                vals[int(k.strip().split("_")[3])] = float(v)
    except OSError:
        pass
    if not vals:
        return None, None
    t = min(vals, key=lambda n: abs(n - threads))
    return vals[t], t


_REAL_STDOUT = None   # a dup of the process's original fd 1 once main() has pointed fd 1 at stderr


def emit(line):
    """The bench line, to the REAL stdout (see main)."""
    sys.stdout.flush()
    if _REAL_STDOUT is None:
        print(line, flush=True)
    else:
        os.write(_REAL_STDOUT, (line + "\n").encode())


def spawn_ranks(n):
    """`python bench.py --gpus N` started WITHOUT a launcher: start the N ranks ourselves, exactly as the task statement's launcher line
    does (one process per GPU, 127.0.0.1 rendezvous on a free port), relay their output and exit with their status."""
    import socket
    import subprocess

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write("bench.py: no launcher environment (RANK / WORLD_SIZE unset) -- spawning " + " ".join(cmd) + "\n")
    return subprocess.call(cmd, env=dict(os.environ, GIGAPOSE_BENCH_SPAWNED="1"))


def traffic_commit():
    """Provenance of the STATIC traffic figure: the commit profiles/pmc_traffic.json was last written at (build
    container: git is there), when tools/pmc_summary.py recorded it, and whether the kernel sources it was recorded on are the ones in
    this tree (sha1 over gigapose_amd/csrc/*.hip + *.h, stamped into the file by pmc_summary.py)."""
    import glob
    import hashlib
    import subprocess

    out = {}
    try:
        r = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h %cs", "--", "profiles/pmc_traffic.json"], capture_output=True, text=True, timeout=10)
        if r.returncode == 0 and r.stdout.strip():
            out["commit"] = r.stdout.strip()
    except Exception:
        pass
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        out["recorded_at"] = pmc.get("_recorded_at")
        if pmc.get("_kernel_sources_sha1"):
            h = hashlib.sha1()
            csrc = os.path.join(ROOT, "gigapose_amd", "csrc")
            for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
                h.update(open(f, "rb").read())
            out["recorded_on_these_kernel_sources"] = h.hexdigest() == pmc["_kernel_sources_sha1"]
    except Exception:
        pass
    return out or None


def matrix_ceiling_on_this_socket():
    """What v_mfma_f32_32x32x16_f16 sustains on THIS socket right now (tools/ubench/mfma_ceiling.hip `brief`: 0.4 s per line, after the
    timed region): MFMA-only loops with all-zero and with random-normal operands, and the 3-product split pattern fed from LDS with its
    reads one step ahead (the structure of gemm_planes256_kernel's k loop, nothing else in the kernel).  The guide's 2495 TFLOP/s is the
    ZERO-data number; real data runs into the socket's 1400 W cap at ~0.65 of it (profiles/r06_ubench_mfma_ceiling.txt).  None if the
    binary is not built (python -c 'import __graft_entry__ as g; g.build()')."""
    import subprocess

    exe = os.path.join(ROOT, "tools", "ubench", "_mfma_ceiling")
    if not os.path.exists(exe):
        return None
    try:
        r = subprocess.run([exe, "brief", "0.4"], capture_output=True, text=True, timeout=60)
    except Exception:
        return None
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("#") or "TFLOP/s" not in ln or "clk" not in ln:
            continue
        try:
            tf = float(ln.split("TFLOP/s")[0].split()[-1])
            mhz = float(ln.split("clk")[1].split()[0])
            watts = float(ln.split("smi:")[1].split()[0]) if "smi:" in ln else 0.0
        except (IndexError, ValueError):   # a reported extra: never lose the bench line over it
            continue
        rec = {"tflops": round(tf, 1), "in_kernel_clock_mhz": round(mhz), "socket_watts": round(watts)}
        if ln.startswith("R  same") and " zeros " in ln:
            out["mfma_only_zero_operands"] = rec
        elif ln.startswith("R  same") and " normal " in ln:
            out["mfma_only_random_operands_same_registers"] = rec
        elif ln.startswith("R  8 + 8") and " normal " in ln:
            out["mfma_only_random_operands"] = rec
        elif ln.startswith("LPP 2x4") and " normal " in ln:
            out["split_pattern_from_lds_random_operands"] = rec
    return out or None


def cpu_baseline(variant, n_templates, k, sample_crops=32, threads=None):
    """The reference's CPU path restated operator for operator in torch (oracle/torch_port.py: HF DINOv2 stand-in forward
    in sub-batches of 4 detections, the 170 MB / detection bank gather, LocalSimilarity.test with its materialised
    similarity tensor, the IST backbone recomputed k times, MLP heads; RANSAC / recovery through the C oracle) on
    `sample_crops` crops of the same workload, onboarding excluded -- what the reference itself executes per crop
    (the unmodified reference measured 1.39 crops/s on 8 threads in the build container)."""
    from transformers import Dinov2Config, Dinov2Model

    from gigapose_testing import factory, synthetic as syn
    from gigapose_amd.vit import VARIANTS
    from oracle import torch_port

    dim, depth, heads = VARIANTS[variant]
    # torch's intra-op pool: the cores this process may run on, capped at 16 (the GPU boxes report 256 logical CPUs of a
    # shared host; 256 threads measured 6 x SLOWER than 8 -- oversubscription; BASELINE.md's reference figure used 8)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = threads or max(1, min(16, avail))
    torch.set_num_threads(threads)
    hf = Dinov2Model(Dinov2Config(hidden_size=dim, num_hidden_layers=depth, num_attention_heads=heads, image_size=224, patch_size=14)).eval()
    ist = factory.build_model("dinov2_vits14", k=k, device="cpu", seed=0).ist_net   # reference-shaped ISTNet mirror (torch modules)
    tset = factory.TemplateSet(1, n_templates, seed=100)
    rs = np.random.RandomState(0)
    # bank values do not change the cost of any operator: random unit features instead of a 57 s/object onboarding pass
    bank_ae = torch.from_numpy(syn._unit(rs.standard_normal((1, n_templates, dim, 16, 16)).astype(np.float32), 2))
    bank_ist = torch.from_numpy(rs.standard_normal((1, n_templates, 256, 16, 16)).astype(np.float32))
    masks = torch.stack([it.mask for it in tset.items])
    geom = syn.template_geometry(101, 1, n_templates)
    q = tset.crops(7, sample_crops, "cpu")
    t0 = time.time()
    torch_port.eval_retrieval(hf, ist, bank_ae, bank_ist, masks, geom, q, k, dets_per_forward=4)
    dt = time.time() - t0
    ratio, ratio_threads = reference_over_port(threads)
    return {"value": round(sample_crops / dt, 4), "unit": "query-crops/sec", "cores": threads, "kind": "port",
            "host_logical_cpus": os.cpu_count(), "cpus_in_affinity_mask": avail,
            # the anchor to the UNMODIFIED reference (which cannot travel to the GPU box): both timed in one process on the same
            # 32 crops / threads in the build container by oracle/time_reference.py -> profiles/r03_cpu_reference_vs_port.txt
            "reference_over_port": ratio,
            "reference_equivalent_value": None if ratio is None else round(ratio * sample_crops / dt, 4),
            "reference_over_port_source": f"profiles/r06_cpu_reference_vs_port.txt: the unmodified reference and this port timed in one process on the same "
                                          f"32 crops x 162 templates at {ratio_threads} torch threads in the build container (idle), oracle/time_reference.py",
            "sample": f"{sample_crops} crops x {n_templates} templates, {variant}, oracle/torch_port.py (torch-CPU restatement of the "
                      f"reference's eval_retrieval, f32, sub-batches of 4, IST backbone x k as the reference recomputes it), "
                      f"torch threads = {threads} (the host reports {os.cpu_count()} logical CPUs, {avail} in this process's affinity mask; "
                      f"more than 16 torch threads measured slower), {dt:.1f} s"}


class _StubLib:
    """Profiling hooks of libgigapose_hip.so with nothing behind them (GIGAPOSE_BENCH_STUB=1, see _StubModel)."""
    class _F:
        restype = None

        def __call__(self, *a):
            return 0

    def __getattr__(self, name):
        if name == "gp_prof_kind_name":
            f = lambda i: [b"gemm_kmajor", b"match", b"attention", b"layernorm", b"conv", b"other", b"gemm_split", b"match_split"][i]
            return f
        return self._F()


class _StubModel:
    """GIGAPOSE_BENCH_STUB=1: everything of THIS FILE -- argument handling, process-group set-up, the timed region with its barriers,
    the max-over-ranks all-reduce, the per-rank gather, the both-modes block, --dump-outputs, the rank-0-only JSON line -- runs on CPU
    over gloo with this object in place of the model (no kernels: `predict` sleeps 2 ms, when sharded issues the two collectives of
    gigapose_amd/sharding.py on small tensors, and returns two small tensors of fixed values).  tests/test_bench_distributed.py
    launches it under torch.distributed.run with two ranks: the 8-GPU driver run must not be the first time this control flow
    executes with more than one rank."""

    def __init__(self):
        import types

        self.template_shard = None
        self.template_datasets = {}
        self.pose_recovery = {}
        self.match_banks = {}
        self.template_datas = {}
        self.overlap_ist = False
        self.testing_metric = types.SimpleNamespace(bank_dtype=None)
        self.ae_net = types.SimpleNamespace(dinov2_model=types.SimpleNamespace(set_split_gemm=lambda m: None))
        self.ist_net = types.SimpleNamespace(backbone=types.SimpleNamespace(conv_kernel="256", invalidate=lambda: None))
        self.numerics = None

    def set_numerics(self, mode):
        self.numerics = mode

    def enable_template_sharding(self, group=None):
        import torch.distributed as dist

        self.template_shard = (dist.get_rank(group), dist.get_world_size(group), group)

    def set_template_data(self, name):
        import types

        self.pose_recovery[name] = types.SimpleNamespace(check_asserts=True)
        self.match_banks[name] = types.SimpleNamespace(hi=torch.zeros(4), lo=None, features=None)
        self.template_datas[name] = object()

    def predict(self, tar_img, *a, **kw):
        import torch.distributed as dist

        from gigapose_amd import sharding
        from gigapose_amd.tensor_collection import TensorCollection

        time.sleep(0.002)
        if self.template_shard is not None and dist.is_initialized():
            rows = torch.zeros(tar_img.shape[0], 64, dtype=torch.uint8)
            allrows, work = sharding.all_gather_rows(rows, self.template_shard[2], async_op=True)   # exchange #1
            if work is not None:
                work.wait()
            sharding.all_to_all_rows(allrows[:, :8].contiguous(), self.template_shard[2])          # exchange #2
        B = tar_img.shape[0]
        return TensorCollection(scores=torch.linspace(0.0, 1.0, B * 5).reshape(B, 5), id_src=torch.arange(B * 5).reshape(B, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="crops per GPU per step")
    ap.add_argument("--objects", type=int, default=1)
    ap.add_argument("--templates", type=int, default=162)
    ap.add_argument("--variant", default="dinov2_vitl14")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--mode", default="auto", choices=["auto", "sharded", "replicas"])
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: roofline and per-family kernel table, matrix-ceiling micro-benchmark, other numerics modes, "
                         "BASELINE config-3 / config-5 shapes and batch curve, drop-in flow, the other multi-GPU mode, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step returned to DIR/<name>.npy (float32 / float64; rank 0's crops when N > 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--overlap", action="store_true", help="IST backbone on a second HIP stream at every batch size (default: up to 32 crops only; at 64 crops measured 0-1 %%)")
    ap.add_argument("--no-configs", action="store_true", help="with --full: skip the BASELINE config-3 / config-5 shaped extra measurements and the drop-in flow")
    ap.add_argument("--no-other", action="store_true", help="with --full: skip timing the other numerics modes")
    ap.add_argument("--numerics", default="split", choices=["split", "chain"],
                    help="numerics of `value`: split = 3 x f16 MFMA on split f32 operands (f32-equivalent, DESIGN.md 2); "
                         "chain = f32-input MFMA fmaf chain (bit-exact vs the CPU oracle).  With --full the other mode is timed too "
                         "and reported under `other_numerics` (N=1 only).")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    stub = os.environ.get("GIGAPOSE_BENCH_STUB") == "1"   # control-flow test of this file on CPU / gloo (see _StubModel); never a measurement
    if not torch.cuda.is_available() and not stub:
        sys.exit("bench.py: no GPU visible -- the hot path is HIP only (no CPU fallback); run it on an MI355X box "
                 "(tests/test_sharding_gloo.py covers the N > 1 exchange logic on CPU)")

    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # ONE JSON line on stdout, whatever the libraries print: RCCL writes a version banner to the C-level stdout when its first
    # communicator is made (seen the first time a driver-style run initialised it, round 6), buffered until exit.  File descriptor 1
    # points at stderr from here on; the JSON line is written to the kept copy of the real stdout at the end.
    global _REAL_STDOUT
    if _REAL_STDOUT is None and ("RANK" in os.environ or args.gpus == 1):   # (a bare --gpus N parent only relays its ranks' output)
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ and os.environ.get("GIGAPOSE_BENCH_SPAWNED") != "1":
        raise SystemExit(spawn_ranks(args.gpus))   # plain `python bench.py --gpus N`: be our own launcher
    if world != args.gpus:
        # one rank per GPU, launched as the task statement says; any other pairing would time a different job than the line reports
        raise SystemExit(f"bench.py --gpus {args.gpus} was started with WORLD_SIZE={world}; launch with: python -m torch.distributed.run "
                         f"--nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 --master-port P bench.py --gpus {args.gpus} ...")
    if stub:
        dev = torch.device("cpu")
        sync = lambda: None
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        sync = torch.cuda.synchronize
    under_launcher = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if world > 1 or (under_launcher and args.mode == "sharded"):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if stub:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    mode = args.mode if args.mode != "auto" else ("sharded" if world > 1 else "single")
    if stub:
        import types

        model = _StubModel()
        _lib = types.SimpleNamespace(check_status=lambda: None)
        factory = None
        tset = None
        q = dict(tar_img=torch.zeros(args.batch, 1), tar_mask=None, tar_K=None, tar_M=None, labels=None)
        lib = _StubLib()
    else:
        from gigapose_amd import _lib
        from gigapose_testing import factory

        model = factory.build_model(args.variant, k=args.k, device=dev, seed=0)
        tset = factory.TemplateSet(args.objects, args.templates, seed=100)
        q = tset.crops(1000 + rank, args.batch, dev)
        lib = _lib.lib()
        lib.gp_prof_kind_name.restype = ctypes.c_char_p
    if mode == "sharded" and dist.is_initialized():
        model.enable_template_sharding()  # world 1: only meaningful with GIGAPOSE_FORCE_COLLECTIVES=1 (path check)
    model.template_datasets = {"syn": tset}
    kinds = 8
    # coprime with the 4 plane-GEMM launches of a ViT layer: the sample cycles through q|k|v, proj, fc1, fc2.  13 (round 6; 5 before): an event pair
    # costs the launch stream ~11 us of idle time around the sampled launch (rocprofv3: 0.21 ms of a 40 ms step at one in 5); ~7 samples per step
    SAMPLE_STRIDE = 13

    def step():
        return model.predict(q["tar_img"], q["tar_mask"], q["tar_K"], q["tar_M"], q["labels"], "syn")

    def timed(steps, profile):
        """profile: None = no events; "all" = HIP events around every launch (per-family table; costs ~3 us per launch);
        ("sampled", kind_name) = events around one in SAMPLE_STRIDE launches of the dominant family only -- what THE timed region uses."""
        if world > 1:
            dist.barrier()
        sync()
        if profile == "all":
            lib.gp_prof_begin(-1, 1)
        elif profile:
            names = [lib.gp_prof_kind_name(i).decode() for i in range(kinds)]
            lib.gp_prof_begin(names.index(profile[1]), SAMPLE_STRIDE)
        t0 = time.perf_counter()
        for _ in range(steps - 1):
            step()
        last = step()   # what the caller of the timed path receives from its last step (--dump-outputs)
        sync()
        t_own = time.perf_counter() - t0   # this rank's own K steps (before the closing barrier): a straggler GPU shows here
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        kern = {}
        if profile:
            ms = (ctypes.c_double * kinds)()
            work = (ctypes.c_double * kinds)()
            cnt = (ctypes.c_longlong * kinds)()
            nk = lib.gp_prof_end(kinds, ms, work, cnt)
            for i in range(nk):
                if cnt[i]:
                    name = lib.gp_prof_kind_name(i).decode()
                    unit = "GB/s" if name == "layernorm" else "TFLOP/s"
                    kern[name] = {"ms_per_step": round(ms[i] / steps, 3), "launches_per_step": cnt[i] // steps,
                                  "avg_launch_us": round(1e3 * ms[i] / cnt[i], 2), "launches_timed": int(cnt[i]),
                                  unit: round(work[i] / ms[i] / (1e6 if name == "layernorm" else 1e9), 2) if ms[i] > 0 else 0.0}
        return dt, kern, t_own, last

    def run_mode(numerics, keep_outputs=False):
        """Onboard the bank in `numerics`, warm up, time K steps (THE timed region), then (--full) replay them with events around every
        launch for the per-family table.  Returns (dt = max over ranks, dt_serial, kernels, sampled kernels, per-rank ms per step,
        the last timed step's outputs on the host if `keep_outputs`)."""
        model.set_numerics(numerics)
        model.set_template_data("syn")  # onboarding: excluded from the timed region (reference gigaPose.py:396-398)
        model.pose_recovery["syn"].check_asserts = False  # no host sync inside the timed loop
        model.overlap_ist = True if args.overlap else "auto"   # "auto" = the product default: the IST backbone on a second stream up to 32 crops only
        for _ in range(args.warmup):
            step()
        # THE timed region: K steps.  --full: HIP events on the launch stream around one in SAMPLE_STRIDE launches of the dominant
        # kernel family (roofline.achieved comes from these).  Bracketing all ~210 launches of a step costs 1.4 ms of queue time per
        # step (measured A/B, 46.3 vs 44.9 ms), so the per-family table comes from a second, untimed replay with full events.
        dominant = "gemm_split" if numerics == "split" else "gemm_kmajor"
        dt, kern_timed, t_own, last = timed(args.steps, profile=("sampled", dominant) if args.full else None)
        _lib.check_status()  # guard rails (lost hand-off / split range / labels): read once, outside the timed region
        outputs = host_outputs(last) if keep_outputs else None   # now: a later predict() may reuse the buffers behind them
        del last
        dt_serial, kern = None, {}
        if args.full:
            overlap = model.overlap_ist
            model.overlap_ist = False
            dt_serial, kern, _, _ = timed(args.steps, profile="all")
            model.overlap_ist = overlap
        per_rank = [round(1e3 * t_own / args.steps, 3)]
        if world > 1:
            tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax.item())
            mine = torch.tensor([t_own], device=dev, dtype=torch.float64)
            every = torch.empty(world, device=dev, dtype=torch.float64)
            dist.all_gather_into_tensor(every, mine)
            per_rank = [round(1e3 * float(t) / args.steps, 3) for t in every.tolist()]
        return dt, dt_serial, kern, kern_timed, per_rank, outputs

    def headline(dt, per_rank_ms):
        """The result line's headline fields: what a plain run prints, and what --full prints ahead of its extras."""
        out = {
            "metric": "query-crops/sec (ViT feat + template NN + 4DoF regress), 162 templates, 1/2/4/8 GPU",
            "value": round(world * args.batch * args.steps / dt, 2), "unit": "query-crops/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32 (ViT linear layers + attention, matcher, IST convolutions: f32 operands split into f16 hi/lo, 3 x f16 MFMA per k-block, f32 accumulate -- "
                      "error vs f64 below the f32 fmaf chain's, tests/test_gpu_split.py; everything else f32)"
                      if args.numerics == "split" else "f32"),
            "data": "synthetic",
            "config": {"workload": f"BASELINE configs[1]: {args.variant} random-init, {args.objects} object(s) x {args.templates} templates, "
                                   f"batch={args.batch} crops per GPU, k={args.k}, full path ViT->match->IST->RANSAC->pose",
                       "numerics": args.numerics, "global_batch": world * args.batch,
                       "parallelism": f"{mode}{world}" if (world > 1 or (mode == "sharded" and dist.is_initialized())) else "single",
                       "streams": ("ViT+match on stream 0, IST backbone on stream 1"
                                   if (model.overlap_ist is True or (model.overlap_ist == "auto" and args.batch <= 32)) else "single stream"),
                       "rccl_ranks": world if dist.is_initialized() else 0,   # = N under the launcher: one rank per GPU
                       "per_rank_ms_per_step": per_rank_ms,                  # each rank's own K steps before the closing barrier (a straggler GPU shows here)
                       "collective_backend": (dist.get_backend() if dist.is_initialized() else None),
                       "host_syncs_in_timed_loop": "none: pose recovery's crop-transform assert readback (reference lib3d/torch.py:54-55) is "
                                                   "disabled for the loop (check_asserts=False); the device status word is read once after it"},
        }
        if stub:
            out["data"] = "STUB (GIGAPOSE_BENCH_STUB=1): control-flow test of bench.py on CPU / gloo, no kernels -- not a measurement"
        return out

    dt, dt_serial, kern, kern_timed, per_rank_ms, outputs = run_mode(args.numerics, keep_outputs=args.dump_outputs is not None and rank == 0)
    if outputs is not None:
        dump_outputs(outputs, args.dump_outputs)
    if not args.full:
        # a plain run: the headline and nothing else
        if rank == 0:
            emit(json.dumps(headline(dt, per_rank_ms)))
        if dist.is_initialized():
            dist.destroy_process_group()
        return
    # N > 1: the same job once more in the OTHER multi-GPU mode, so that one driver run reports both -- "sharded" (north_star's
    # template-bank partition: two exchanges per step) and "replicas" (full bank per GPU, no data-path collective).  Weak scaling
    # either way; in sharded mode every rank still matches all W * B crops against its 1 / W of the bank, so it saves memory,
    # not matcher work.  The switch is the same on every rank (it depends on world / mode only): the collectives stay paired.
    other_modes = None
    stuck_group = False
    if (world > 1 or os.environ.get("GIGAPOSE_BENCH_BOTH_MODES") == "1") and mode in ("sharded", "replicas"):   # env: exercise the block at world 1
        alt = "replicas" if mode == "sharded" else "sharded"
        err = None
        try:
            if alt == "replicas":
                model.template_shard = None
            else:
                model.enable_template_sharding()
            adt, _, akern, _, aper, _ = run_mode(args.numerics)
            other_modes = {alt: {"value": round(world * args.batch * args.steps / adt, 2), "unit": "query-crops/sec",
                                 "ms_per_step": round(1e3 * adt / args.steps, 3), "parallelism": f"{alt}{world}",
                                 "per_rank_ms_per_step": aper,
                                 "kernels_ms_per_step": {k: v["ms_per_step"] for k, v in akern.items()}}}
        except Exception as e:  # never lose the headline line
            err = repr(e)
            other_modes = {alt: {"error": err}}
        if world > 1:
            # a rank that failed alone has left its peers inside a collective of the second pass: say so on every rank instead of
            # hanging -- the flag exchange itself cannot pair with a data-path collective (those are finished or dead by now)
            # (bounded: a peer that is STILL inside a data-path collective never reaches this exchange -- give up after 60 s and
            # report instead of hanging the headline line)
            flag = torch.tensor([1 if err else 0], device=dev, dtype=torch.int32)
            work = dist.all_reduce(flag, op=dist.ReduceOp.MAX, async_op=True)
            deadline = time.time() + 60.0
            while not work.is_completed() and time.time() < deadline:
                time.sleep(0.01)
            if not work.is_completed():
                other_modes = {alt: {"error": (err or "") + " | failure-flag exchange timed out after 60 s (a peer is stuck in a collective)"}}
                if rank == 0:   # the headline measurement is complete: print it and leave without joining the dead group
                    stuck_group = True
                else:
                    os._exit(0)
            else:
                work.wait()
                if int(flag.item()) and not err:
                    other_modes = {alt: {"error": "another rank failed in this mode"}}
    other = None
    if world == 1 and not dist.is_initialized() and not args.no_other and not stub:
        other = {}

        def numerics_entry(name, odt, odt_serial, okern, note=None):
            e = {"numerics": name, "value": round(args.batch * args.steps / odt, 2), "unit": "query-crops/sec",
                 "ms_per_step": round(1e3 * odt / args.steps, 3), "replay_ms_per_step_with_all_events": round(1e3 * odt_serial / args.steps, 3),
                 "kernels": okern}
            if note:
                e["note"] = note
            return e

        other_mode = "chain" if args.numerics == "split" else "split"
        try:
            odt, odt_serial, okern, _, _, _ = run_mode(other_mode)
            other[other_mode] = numerics_entry(other_mode, odt, odt_serial, okern,
                                               "verification mode: f32-input MFMA fmaf chains, bit-exact vs the CPU oracle" if other_mode == "chain" else None)
        except Exception as e:
            other[other_mode] = {"error": repr(e)}
        # split128: what the automatic range fallback lands in (gigaPose.py: _widen_split_range) when a checkpoint's activations
        # leave the x8 f16 planes' range (|x| >= 8190): ViT linear layers + IST convolutions on the two-accumulator 128 x 128
        # kernels (Dinov2ViT.set_split_gemm("128") + ResNet.conv_kernel = "128"), everything else as in split
        vit, ist = model.ae_net.dinov2_model, model.ist_net.backbone   # bound BEFORE the try: the finally below restores them
        try:
            vit.set_split_gemm("128")
            ist.conv_kernel = "128"
            ist.invalidate()
            odt, odt_serial, okern, _, _, _ = run_mode("split")
            other["split128"] = numerics_entry("split128", odt, odt_serial, okern,
                                               "the mode the automatic range fallback selects (|activation| >= 8190): 128 x 128 two-accumulator kernels, range 65504")
        except Exception as e:
            other["split128"] = {"error": repr(e)}
        finally:
            vit.set_split_gemm("256")
            ist.conv_kernel = "256"
            ist.invalidate()
        # split_outliers: the same model with DINOv2-like planted outliers (gigapose_testing/synthetic.py: OUTLIER_SPEC -- massive GELU
        # activations in two layers, a value-projection channel at 9e3, LayerNorm gains of 600 on residual outlier channels): the
        # default x 8 planes would trip the range guard; onboarding calibrates per-tensor plane scales on the templates and every
        # GEMM stays on the 256 x 256 plane kernels (round 4 landed in split128 for such weights)
        try:
            from gigapose_testing import synthetic as syn_

            vit = model.ae_net.dinov2_model
            keep_sd = {k: v.detach().clone() for k, v in vit.state_dict().items()}
            syn_.plant_dinov2_outliers(vit)
            try:
                odt, odt_serial, okern, _, _, _ = run_mode("split")
                e = numerics_entry("split_outliers", odt, odt_serial, okern,
                                   "planted DINOv2-like outliers; per-tensor plane scales calibrated at onboarding (vit.py: calibrate_plane_scales), "
                                   "all GEMMs on the 256 x 256 plane kernels")
                e["plane_scales_not_8"] = {k: {"max_abs": round(a, 1), "scale": sc} for k, (a, sc) in vit.plane_scale_report().items()}
                e["split_gemm"] = vit.split_gemm
                other["split_outliers"] = e
            finally:
                vit.load_state_dict(keep_sd)
        except Exception as e:
            other["split_outliers"] = {"error": repr(e)}
        model.set_numerics(args.numerics)
        for key in ("split128", "split_outliers"):
            if isinstance(other.get(key), dict) and "value" in other[key]:
                other[key]["relative_to_headline"] = round(other[key]["value"] / (args.batch * args.steps / dt), 3)
    # BASELINE configs 3 and 5 at size on this one GPU (N = 1 only): same path, headline numerics, fewer steps.  Config 5's
    # bank is the fp16 (hi-plane-only) one its text asks for; at N = 8 it would be sharded 8-way (1/8 of these bytes per GPU).
    # Config 3 also at B = 128 (B = 64 and 128) and as a batch curve B = 8 / 16 / 32 (the reference forwards
    # detections 4 at a time, configs/test.yaml:21; a frame holds up to 16 per object id, dataloader/test.py:104-107).
    other_configs = batch_curve = None
    if world == 1 and not dist.is_initialized() and not args.no_configs and args.variant == "dinov2_vitl14" and not stub:
        other_configs, batch_curve = {}, {}

        def onboard(key, n_obj, bank_dtype):
            tset_c = factory.TemplateSet(n_obj, args.templates, seed=300 + n_obj)
            model.set_numerics(args.numerics)
            model.testing_metric.bank_dtype = bank_dtype
            model.template_datasets = {key: tset_c}
            t0 = time.perf_counter()
            model.set_template_data(key)
            t_onboard = time.perf_counter() - t0
            model.pose_recovery[key].check_asserts = False
            return tset_c, t_onboard

        def time_batch(key, tset_c, n_obj, batch, n_steps):
            qc = tset_c.crops(2000 + n_obj, batch, dev)
            run = lambda: model.predict(qc["tar_img"], qc["tar_mask"], qc["tar_K"], qc["tar_M"], qc["labels"], key)
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                run()
            torch.cuda.synchronize()
            dtc = time.perf_counter() - t0
            _lib.check_status()
            return {"value": round(batch * n_steps / dtc, 2), "unit": "query-crops/sec", "batch": batch, "steps": n_steps,
                    "ms_per_step": round(1e3 * dtc / n_steps, 3)}

        def drop(key):
            model.match_banks.pop(key, None)
            model.template_datas.pop(key, None)
            model.pose_recovery.pop(key, None)
            torch.cuda.empty_cache()

        n_half = max(3, args.steps // 2)
        # config 3 (LM-O shape): B = 64, B = 128, and the batch curve -- one onboarding
        try:
            text3 = "LM-O shape: 8 objects x 162 templates, multi-detection batch with mixed labels, 1 GPU"
            tset3, t_on = onboard("config3", 8, "f32")
            bank = model.match_banks["config3"]
            nbytes = sum(t.numel() * t.element_size() for t in (bank.hi, bank.lo, bank.features) if t is not None)
            common = {"numerics": args.numerics, "bank_dtype": "f32", "matcher_bank_GB": round(nbytes / 1e9, 3),
                      "onboarding_s_per_object": round(t_on / 8, 3)}
            r64 = time_batch("config3", tset3, 8, args.batch, n_half)
            other_configs["config3"] = {"workload": text3 + f", batch={args.batch}", **r64, **common}
            try:
                r128 = time_batch("config3", tset3, 8, 2 * args.batch, n_half)
                other_configs["config3_b128"] = {"workload": text3 + f", batch={2 * args.batch} (SURVEY 8(d): B = 64 and 128)", **r128, **common}
            except Exception as e:
                other_configs["config3_b128"] = {"error": repr(e)}
            try:
                per_crop_64 = r64["value"]
                for bsz in (8, 16, 32):
                    r = time_batch("config3", tset3, 8, bsz, 5)
                    r["per_crop_rate_vs_b64"] = round(r["value"] / per_crop_64, 3)
                    batch_curve[f"b{bsz}"] = r
                batch_curve["workload"] = text3 + "; crops/s at B = 8 / 16 / 32 (5 steps each, product default = IST backbone on a second stream) and their ratio to the B = 64 rate of the same bank"
                batch_curve[f"b{args.batch}"] = {"value": r64["value"], "batch": args.batch, "ms_per_step": r64["ms_per_step"]}
                # b8 / b16 / b32 above ran the product default (GigaPose.overlap_ist = "auto": the IST backbone on a second HIP stream up to
                # 32 crops -- below 64 crops neither chain fills the chip); the same three on ONE stream for comparison
                keep = model.overlap_ist
                try:
                    model.overlap_ist = False
                    for bsz in (8, 16, 32):
                        r = time_batch("config3", tset3, 8, bsz, 5)
                        r["per_crop_rate_vs_b64"] = round(r["value"] / per_crop_64, 3)
                        batch_curve[f"b{bsz}_single_stream"] = r
                except Exception as e:
                    batch_curve["single_stream_error"] = repr(e)
                finally:
                    model.overlap_ist = keep
            except Exception as e:
                batch_curve["error"] = repr(e)
            drop("config3")
            del tset3
        except Exception as e:  # an extra measurement must never cost the headline line
            other_configs["config3"] = {"error": repr(e)}
        if args.numerics == "split":   # the fp16 (hi-plane-only) bank exists in split numerics only
            try:
                tset5, t_on = onboard("config5", 40, "f16")
                bank = model.match_banks["config5"]
                nbytes = sum(t.numel() * t.element_size() for t in (bank.hi, bank.lo, bank.features) if t is not None)
                other_configs["config5"] = {"workload": "HANDAL/HOPE scale: 40 objects x 162 templates, fp16 feature bank resident in HBM, 1 GPU "
                                                        f"(unsharded replica), batch={args.batch}",
                                            **time_batch("config5", tset5, 40, args.batch, n_half), "numerics": args.numerics, "bank_dtype": "f16",
                                            "matcher_bank_GB": round(nbytes / 1e9, 3), "onboarding_s_per_object": round(t_on / 40, 3),
                                            "parity": "bounded, not exact: the f16-rounded template features flip ~10 of 2.65 M patch ids and 4 of 64 "
                                                      "top-5 sets end to end (tests/test_gpu_parity_big.py); the f32-class bank (6.8 GB) is the parity mode"}
                drop("config5")
                del tset5
            except Exception as e:
                other_configs["config5"] = {"error": repr(e)}
        model.testing_metric.bank_dtype = None
        model.template_datasets = {"syn": tset}
    # The drop-in flow (N = 1 only): what `trainer.test` of the reference's test.py drives -- ONE image per test_step (reference
    # test.py:55-60), 8 detections per image here, 64 images.  accumulated: the product default (GigaPose.accumulate_crops = 64: whole
    # images queued, one predict per 64 pending crops, per-image npz files written while the next flush runs); per_image: the
    # reference's flow (accumulate_crops = 0: one predict + file per image).  Wall clock from the first test_step to the last file.
    dropin_flow = None
    if world == 1 and not dist.is_initialized() and not args.no_configs and not stub:
        try:
            import shutil
            import tempfile

            import pandas as pd

            from gigapose_amd.tensor_collection import PandasTensorCollection

            model.set_numerics(args.numerics)
            model.template_datasets = {"syn": tset}
            model.set_template_data("syn")
            model.test_dataset_name = "syn"
            n_img, n_det = 64, 8
            images = []
            for im in range(n_img):
                qi = tset.crops(5000 + im, n_det, dev)
                lab = qi["labels"].numpy()
                b = PandasTensorCollection(infos=pd.DataFrame(dict(label=[str(l) for l in lab], scene_id=[1] * n_det, view_id=[im] * n_det)),
                                           **{k: qi[k] for k in ["tar_img", "tar_mask", "tar_K", "tar_M"]})
                objs = sorted(set(int(l) for l in lab))
                b.test_list = PandasTensorCollection(infos=pd.DataFrame(dict(im_id=[im] * len(objs), scene_id=[1] * len(objs), obj_id=objs,
                                                                             inst_count=[int((lab == o).sum()) for o in objs],
                                                                             detection_time=[0.0] * len(objs))))
                images.append(b)
            keep_dir, keep_acc = model.log_dir, model.accumulate_crops
            dropin_flow = {"workload": f"{n_img} images x {n_det} detections through GigaPose.test_step (one image per call, as the reference's "
                                       f"test.py feeds it) + the final flush; headline bank ({args.objects} object(s) x {args.templates} templates), "
                                       "per-image npz files written", "numerics": args.numerics}
            # per_image_pipelined: accumulate_crops = 1 -- every image is its own predict() (the reference's batches), but queued like a
            # flush: its files are written while the next image runs on the GPU
            for name, acc in (("accumulated", 64), ("per_image", 0), ("per_image_pipelined", 1)):
                tmp = tempfile.mkdtemp(prefix="gigapose_flow_")
                try:
                    model.log_dir, model.accumulate_crops = tmp, acc
                    os.makedirs(os.path.join(tmp, "predictions"), exist_ok=True)
                    for b in images[:8]:          # warm-up: one flush / eight images
                        model.test_step(b, 9999)
                    model.flush_pending()
                    passes = []
                    for _ in range(3):   # three passes, the median counts: one np.savez in a few hundred stalls for ~50 ms on these hosts' /tmp
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for im, b in enumerate(images):
                            model.test_step(b, im)
                        model.flush_pending()
                        torch.cuda.synchronize()
                        passes.append(time.perf_counter() - t0)
                    dtf = sorted(passes)[1]
                    n_files = len([f for f in os.listdir(os.path.join(tmp, "predictions")) if f.endswith(".npz")])
                    dropin_flow[name] = {"value": round(n_img * n_det / dtf, 2), "unit": "query-crops/sec", "accumulate_crops": acc,
                                         "ms_per_image": round(1e3 * dtf / n_img, 3), "npz_files_written": n_files - 1,
                                         "passes_crops_per_s": [round(n_img * n_det / t, 1) for t in passes]}
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
            # sharded_forced_world1: the SAME flow with a template-sharded model -- fixed 64-row flushes through sharded_flow.py, a
            # one-rank RCCL group with the collectives forced (GIGAPOSE_FORCE_COLLECTIVES=1): exchange #1 (all_gather_into_tensor of
            # the query rows + the done words), exchange #2 (all_to_all_single), the status-word all-gather all run through the
            # nccl backend on device buffers, so this line exercises the N > 1 code path on the one GPU the driver's bench has
            tmp = tempfile.mkdtemp(prefix="gigapose_flow_")
            keep_env = os.environ.get("GIGAPOSE_FORCE_COLLECTIVES")
            try:
                import socket

                sk = socket.socket()
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
                sk.close()
                os.environ["GIGAPOSE_FORCE_COLLECTIVES"] = "1"
                dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
                model.enable_template_sharding()
                model.template_datas, model.match_banks, model.pose_recovery = {}, {}, {}
                model.set_template_data("syn")
                model.log_dir, model.accumulate_crops = tmp, 64
                os.makedirs(os.path.join(tmp, "predictions"), exist_ok=True)
                for b in images[:8]:
                    model.test_step(b, 9999)
                model.flush_pending()
                passes = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for im, b in enumerate(images):
                        model.test_step(b, im)
                    model.flush_pending()
                    torch.cuda.synchronize()
                    passes.append(time.perf_counter() - t0)
                dtf = sorted(passes)[1]
                n_files = len([f for f in os.listdir(os.path.join(tmp, "predictions")) if f.endswith(".npz")])
                dropin_flow["sharded_forced_world1"] = {
                    "value": round(n_img * n_det / dtf, 2), "unit": "query-crops/sec", "accumulate_crops": 64, "ms_per_image": round(1e3 * dtf / n_img, 3),
                    "npz_files_written": n_files - 1, "passes_crops_per_s": [round(n_img * n_det / t, 1) for t in passes], "rccl_ranks": 1,
                    "note": "includes the one all-dummy flush every drain ends with (the ranks learn that all queues are empty one flush late)"}
            except Exception as e:
                dropin_flow["sharded_forced_world1"] = {"error": repr(e)}
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
                if keep_env is None:
                    os.environ.pop("GIGAPOSE_FORCE_COLLECTIVES", None)
                else:
                    os.environ["GIGAPOSE_FORCE_COLLECTIVES"] = keep_env
                model.template_shard, model._sharded_flow = None, None
                model.template_datas, model.match_banks, model.pose_recovery = {}, {}, {}
                if dist.is_initialized():
                    dist.destroy_process_group()
                model.set_template_data("syn")   # the unsharded bank again (the roofline block below reads its masks)
            model.log_dir, model.accumulate_crops = keep_dir, keep_acc
            if "value" in dropin_flow.get("sharded_forced_world1", {}):
                dropin_flow["sharded_over_b64_rate"] = round(dropin_flow["sharded_forced_world1"]["value"] / (world * args.batch * args.steps / dt), 3)
            dropin_flow["accumulated_over_b64_rate"] = round(dropin_flow["accumulated"]["value"] / (world * args.batch * args.steps / dt), 3)
            dropin_flow["accumulated_over_per_image"] = round(dropin_flow["accumulated"]["value"] / dropin_flow["per_image"]["value"], 3)
        except Exception as e:
            dropin_flow = {"error": repr(e)}
    if rank != 0:
        dist.destroy_process_group()
        return

    # HBM traffic of the dominant kernel family from the committed PMC passes of this same command (tools/pmc_bench.sh;
    # counters cannot be collected from inside the timed run): bytes per launch, corrected as the MI355X guide says
    traffic = None
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        if args.variant == "dinov2_vitl14" and args.batch == 64 and args.templates == 162:
            fam = ("gemm_planes" if "gemm_planes" in pmc else "gemm_split") if args.numerics == "split" else "gemm_kmajor"
            traffic = round(pmc[fam]["hbm_bytes_per_launch"])
    except Exception:
        pass
    F16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X dense f16/bf16 MFMA peak (MI355X_MICROARCH.md); assumes the 2.4 GHz maximum clock
    PEAK_CLOCK_MHZ = 2400.0
    if args.numerics == "split":
        g = kern_timed.get("gemm_split", {})   # the sampled launches of THE timed region
        alg = g.get("TFLOP/s", 0.0)            # algorithmic 2 I J K flops of the launches / their event-timed duration
        executed = round(3.0 * alg, 2)         # what the matrix core executes: 3 f16 MFMAs per f32-equivalent product block
        ceil = None if stub else matrix_ceiling_on_this_socket()
        roofline = {"kernel": "gemm_planes256_kernel (ViT linear layers; 3 x v_mfma_f32_32x32x16_f16 per k-block on f16-split f32 "
                              "operands held as hi / lo planes, f32 accumulate)", "bound": "mfma",
                    # achieved / frac: USEFUL work against the roofline, as SURVEY 8(d) defines it (162 GFLOP / crop figure -> 2 I J K per
                    # launch); the split emulation's 3 executed flops per useful flop are reported beside it, not in it
                    "achieved": alg, "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(alg / F16_MFMA_PEAK_TFLOPS, 4),
                    "achieved_is": "algorithmic f32-equivalent flops (2 I J K per launch) / event-timed launch duration",
                    "executed_tflops": executed,
                    "mfma_util_executed": round(executed / F16_MFMA_PEAK_TFLOPS, 4),
                    # round 6: the ceiling is MEASURED on this socket, after the timed region, by an MFMA-only loop on random data (the
                    # guide's 2495 TFLOP/s reproduces with all-zero operands only; random data hits the 1400 W cap at ~0.65 of it)
                    "sustained_mfma_only_tflops": (ceil or {}).get("mfma_only_random_operands", {}).get("tflops"),
                    "sustained_split_pattern_tflops": (ceil or {}).get("split_pattern_from_lds_random_operands", {}).get("tflops"),
                    "executed_over_sustained_mfma_only": (round(executed / ceil["mfma_only_random_operands"]["tflops"], 4)
                                                          if ceil and "mfma_only_random_operands" in ceil else None),
                    "matrix_ceiling_ubench": ceil,
                    "frac_vs_f32_input_mfma_peak": round(alg / F32_MFMA_PEAK_TFLOPS, 3),
                    "note": "frac = useful (algorithmic) flops / f16 dense peak.  mfma_util_executed = 3 x that: the three f16 products per "
                            "f32-equivalent product all execute on the matrix core (north_star's MFMA-utilisation reading).  "
                            "sustained_mfma_only_tflops: v_mfma_f32_32x32x16_f16 alone on random-normal operands, whole chip, 0.4 s, measured by "
                            "tools/ubench/mfma_ceiling.hip right after the timed region -- the socket's power cap, not the 2.4 GHz clock, sets "
                            "it (all-zero operands reach the guide's 2495); sustained_split_pattern_tflops: the same for the 3-product pattern "
                            "with its 12 LDS fragment reads per 24 MFMAs.  executed_over_sustained_mfma_only = executed_tflops / the former: "
                            "how much of what this socket can do on real data the whole kernel (epilogues, strip, prologue included) delivers.  "
                            "frac_vs_f32_input_mfma_peak: the same useful flops against the 157.3 TFLOP/s f32-input MFMA peak the reference's "
                            "dtype would otherwise be bound by",
                    "traffic": traffic}
    else:
        g = kern_timed.get("gemm_kmajor", {})
        achieved = g.get("TFLOP/s", 0.0)
        roofline = {"kernel": "gemm_kmajor_kernel (ViT linear layers + IST MLP; f32-input MFMA 32x32x2)", "bound": "mfma",
                    "achieved": achieved, "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(achieved / F32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic}
    if args.numerics == "split" and not stub and "match_split" in kern:
        try:
            from gigapose_amd.matching import patch_grid_mask

            bank = model.match_banks["syn"]
            bm = getattr(bank, "shard", bank).masks                                     # (O, N, 256)
            qlive = (patch_grid_mask(q["tar_mask"]) != 0).sum(-1)                        # (B,)
            tlive = (bm[(q["labels"].to(bm.device) - 1).long()] != 0).sum(-1)            # (B, N)
            blocks = (((qlive + 31) // 32)[:, None] * ((tlive + 31) // 32)).float().mean().item()
            m = kern["match_split"]
            m["nominal_TFLOP/s"] = m["TFLOP/s"]                                         # 2 x 256 x 256 x C per tile, masked-out patches included
            m["live_block_fraction"] = round(blocks / 64.0, 4)                          # 32 x 32 blocks the kernel multiplies / 64
            m["executed_TFLOP/s"] = round(3.0 * m["TFLOP/s"] * blocks / 64.0, 2)        # f16 MFMA flops actually issued
            m["mfma_util_executed"] = round(m["executed_TFLOP/s"] / F16_MFMA_PEAK_TFLOPS, 4)
            m["note"] = ("TFLOP/s is NOMINAL (every patch of the 256 x 256 tile); the kernel multiplies only the 32 x 32 blocks that hold live "
                         "(unmasked) patches: executed = 3 x nominal x live_block_fraction")
        except Exception as e:
            kern["match_split"]["executed_note"] = "not computed: " + repr(e)
    roofline.update({
        "traffic_unit": "bytes per launch (2 x FETCH_SIZE + WRITE_SIZE); algorithmic operand + result bytes per launch: DESIGN.md section 4",
        "traffic_source": "STATIC: read from profiles/pmc_traffic.json, the rocprofv3 --pmc passes of this same command recorded by "
                          "tools/pmc_bench.sh (separate FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 correction) -- PMC counters cannot be "
                          "collected inside the timed run",
        "traffic_commit": traffic_commit(),
        "share_of_step": round(kern.get("gemm_split" if args.numerics == "split" else "gemm_kmajor", {}).get("ms_per_step", 0.0)
                               / (1e3 * dt_serial / args.steps), 3),
        "measured": f"live in THE timed region: HIP events on the launch stream around one in {SAMPLE_STRIDE} launches of this kernel family "
                    f"({g.get('launches_timed', 0)} launches, average {g.get('avg_launch_us', 0)} us; the stride cycles through the four "
                    "GEMM shapes of a layer).  `kernels` = a second, UNTIMED replay of the same steps with events around every launch "
                    "(bracketing all ~210 launches of a step costs 1.4 ms of queue time per step, so it is kept out of `value`)",
        "replay_ms_per_step_with_all_events": round(1e3 * dt_serial / args.steps, 3), "kernels": kern,
        "timed_region_sample": {k: {"launches_timed": v["launches_timed"], "avg_launch_us": v["avg_launch_us"]} for k, v in kern_timed.items()}})
    out = headline(dt, per_rank_ms)
    out["roofline"] = roofline
    if other_modes is not None:
        out["other_modes"] = other_modes
    if other is not None:
        out["other_numerics"] = other
    if other_configs:
        out["other_configs"] = other_configs
    if batch_curve:
        out["batch_curve"] = batch_curve
    if dropin_flow:
        out["dropin_flow"] = dropin_flow
    if world == 1 and not args.no_cpu_baseline and not stub:
        try:
            out["cpu_baseline"] = cpu_baseline(args.variant, args.templates, args.k)
        except Exception as e:  # the baseline is a reported extra; never lose the GPU number
            out["cpu_baseline"] = {"error": repr(e)}
    emit(json.dumps(out))
    if stuck_group:
        os._exit(0)   # a peer never left a collective: destroy_process_group() would wait for it
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
