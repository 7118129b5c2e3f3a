"""layernorm_planes_reg_kernel: launch time against the number of 32-token blocks (two blocks are resident per CU = 512 slots; the ViT-L
step at 64 crops has 16640 rows of which 16448 = 514 blocks carry tokens).  First column pairs: every row live (what the stage entry
runs by itself); last lines: the forward's shape with its live-token count (probe library: gp_vit_set_ln_live) -- the six blocks of
row padding do not run and the two blocks past the round ride on first-round blocks."""

import torch

from gigapose_amd import _lib

_lib.use_probe_library()
dev = torch.device("cuda", 0)
C = 1024
g = torch.randn(C, device=dev)
b = torch.randn(C, device=dev)


def measure(Mpad, live):
    X = torch.randn(C, Mpad, device=dev)
    hi = torch.empty(Mpad, C, dtype=torch.float16, device=dev)
    lo = torch.empty_like(hi)

    def run():
        _lib.call("gp_layernorm_planes", X, hi, lo, g, b, C, Mpad, 1e-6, _lib.stream_ptr())

    _lib.value("gp_vit_set_ln_live", live)
    try:
        for _ in range(5):
            run()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(40):
                run()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 40 * 1e3)
    finally:
        _lib.value("gp_vit_set_ln_live", 0)
    return best


print("# blocks  Mpad   us/launch   GB/s (8 C Mpad bytes)")
for blocks in (256, 384, 448, 504, 512, 514, 520, 528, 544, 576, 640, 768, 1024, 1040):
    Mpad = 32 * blocks
    best = measure(Mpad, 0)
    print(f"{blocks:7d} {Mpad:6d} {best:9.2f} {8.0 * C * Mpad / best / 1e3:9.0f}")
print("# live blocks  Mpad   us/launch   (the forward's launch: rows past the live tokens are padding)")
for live_blocks, Mpad in ((514, 16640), (513, 16640), (516, 16640), (512, 16640), (520, 16640)):
    print(f"{live_blocks:12d} {Mpad:6d} {measure(Mpad, 32 * live_blocks):9.2f}")
_lib.check_status()
