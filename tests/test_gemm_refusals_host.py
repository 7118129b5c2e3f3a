"""CPU: what the five GEMM entry points refuse (include/gigapose_hip.h states each requirement), on the product and the probe library.

A refusal is an argument check: it returns -1 and names the violated requirement in gp_last_error() BEFORE any HIP call, so it needs no
device -- and on a machine without one every accepted call fails too (-2, a launch failure), which is why each case asserts the message and
not the code alone.  The pointers are made-up aligned addresses (a refused call dereferences nothing); with a device visible an accepted
call would launch on them, so the module runs only where there is none.  One case per guard; `base` arguments are a call every guard
accepts, each case changes what its guard looks at."""
import pytest
import torch

from gigapose_amd import _lib

if torch.cuda.is_available():
    pytest.skip("made-up device addresses: only where no device is visible", allow_module_level=True)

P = [0x7f0000000000 + n * 0x100000000 for n in range(12)]   # twelve 16-byte aligned addresses, 4 GiB apart

KMAJOR = ("A", "lda", "B", "ldb", "D", "ldd", "I", "J", "K", "epilogue", "bias", "scale", "residual", "ldr")
SPLIT = ("act", "ld_act", "whi", "wlo", "D", "ldd", "I", "J", "K", "act_is_b", "epilogue", "bias", "scale", "residual", "ldr")
PLANES = ("a_hi", "a_lo", "b_hi", "b_lo", "D", "ldd", "out_hi", "out_lo", "ldo", "I", "J", "J_valid", "K", "epilogue", "bias", "scale",
          "residual", "ldr", "out_scale", "plane_scale", "amax")
ENTRIES = {   # name -> (parameters before the scratch / stream tail, has a scratch, base arguments)
    "gp_gemm_kmajor": (KMAJOR, False, dict(A=P[0], lda=256, B=P[1], ldb=384, D=P[2], ldd=384, I=256, J=384, K=80, epilogue=3, bias=P[3],
                                           scale=P[4], residual=P[5], ldr=384)),
    "gp_gemm_kmajor_sk": (KMAJOR, True, dict(A=P[0], lda=256, B=P[1], ldb=384, D=P[2], ldd=384, I=256, J=384, K=80, epilogue=3, bias=P[3],
                                             scale=P[4], residual=P[5], ldr=384)),
    "gp_gemm_split": (SPLIT, False, dict(act=P[0], ld_act=384, whi=P[1], wlo=P[2], D=P[3], ldd=384, I=256, J=384, K=96, act_is_b=1,
                                         epilogue=3, bias=P[4], scale=P[5], residual=P[6], ldr=384)),
    "gp_gemm_split256": (SPLIT, True, dict(act=P[0], ld_act=16640, whi=P[1], wlo=P[2], D=P[3], ldd=16640, I=1024, J=16640, K=96,
                                           act_is_b=1, epilogue=3, bias=P[4], scale=P[5], residual=P[6], ldr=16640)),
    "gp_gemm_planes256_scaled": (PLANES, True, dict(a_hi=P[0], a_lo=P[1], b_hi=P[2], b_lo=P[3], D=P[4], ldd=16640, out_hi=P[5], out_lo=P[6],
                                                    ldo=1024, I=1024, J=16640, J_valid=16448, K=64, epilogue=3, bias=P[7], scale=P[8],
                                                    residual=P[9], ldr=16640, out_scale=1.0 / 512, plane_scale=8.0, amax=0)),
}
WORKSPACE = {"gp_gemm_kmajor_sk": "gp_gemm_streamk_workspace_bytes", "gp_gemm_split256": "gp_gemm_split256_workspace_bytes",
             "gp_gemm_planes256_scaled": "gp_gemm_split256_workspace_bytes"}
PLANES7 = dict(epilogue=7, D=0, ldd=0, residual=0, ldr=0, scale=0)   # the q | k | v launch: plane outputs, no f32 operand

NEW = "guard added with this module"     # the others stood before it -- those of gp_gemm_split256 and gp_gemm_planes256_scaled behind the
                                         # reset of the scratch, a HIP call: without a device they answered -2 and no message
CASES = [   # (entry, what changes, a substring of the message that names the requirement, NEW or None)
    # ---- gp_gemm_kmajor / gp_gemm_kmajor_sk (one launcher)
    ("gp_gemm_kmajor", dict(K=0), "empty problem", None),
    ("gp_gemm_kmajor", dict(I=100), "multiples of 128", None),
    ("gp_gemm_kmajor", dict(lda=258), "bad leading dimensions lda=258", None),
    ("gp_gemm_kmajor", dict(lda=252), "bad leading dimensions lda=252", None),
    ("gp_gemm_kmajor", dict(ldb=380), "bad leading dimensions lda=256 ldb=380", None),
    ("gp_gemm_kmajor", dict(ldd=380), "bad leading dimensions lda=256 ldb=384 ldd=380", None),
    ("gp_gemm_kmajor", dict(I=65536, lda=65536, ldd=32768, J=128, ldb=128, ldr=128), "larger than 2^31 elements", None),
    ("gp_gemm_kmajor", dict(B=0), "null pointer", None),
    ("gp_gemm_kmajor", dict(A=P[0] + 4), "operands must be 16-byte aligned", None),
    ("gp_gemm_kmajor", dict(epilogue=1, bias=0), "bias required", None),
    ("gp_gemm_kmajor", dict(residual=0), "bias/scale/residual required", None),
    ("gp_gemm_kmajor", dict(ldr=380), "ldr=380 is below J=384", None),
    ("gp_gemm_kmajor", dict(epilogue=9), "unknown epilogue 9", None),
    ("gp_gemm_kmajor_sk", dict(scratch=0), "scratch too small", None),
    ("gp_gemm_kmajor_sk", dict(scratch_bytes=4096), "scratch too small", None),
    ("gp_gemm_kmajor_sk", dict(scratch=P[11] + 4), "scratch must be 16-byte aligned", None),
    ("gp_gemm_kmajor_sk", dict(ldd=380), "bad leading dimensions", None),
    # ---- gp_gemm_split
    ("gp_gemm_split", dict(K=80), "multiples of 128 and K=80 of 32", None),
    ("gp_gemm_split", dict(wlo=0), "null / misaligned operand", None),
    ("gp_gemm_split", dict(act=P[0] + 8), "null / misaligned operand", None),
    ("gp_gemm_split", dict(ld_act=386), "null / misaligned operand", None),
    ("gp_gemm_split", dict(I=65536, ldd=32768, J=128, ld_act=128, ldr=128), "output too large", None),
    ("gp_gemm_split", dict(ld_act=380), "ld_act=380 is below the activation extent 384", NEW),
    ("gp_gemm_split", dict(act_is_b=0, ld_act=252), "ld_act=252 is below the activation extent 256", NEW),
    ("gp_gemm_split", dict(ldd=380), "ldd=380 is below J=384", NEW),
    ("gp_gemm_split", dict(epilogue=1, bias=0), "epilogue 1 needs a bias", NEW),
    ("gp_gemm_split", dict(epilogue=4, bias=0), "epilogue 4 needs a bias", NEW),
    ("gp_gemm_split", dict(epilogue=5, bias=P[4] + 4), "bias must be 16-byte aligned", NEW),
    ("gp_gemm_split", dict(scale=0), "epilogue 3 needs scale and residual", NEW),
    ("gp_gemm_split", dict(residual=0), "epilogue 3 needs scale and residual", NEW),
    ("gp_gemm_split", dict(ldr=380), "ldr=380 is below J=384", NEW),
    ("gp_gemm_split", dict(epilogue=9), "unknown epilogue 9", None),
    # ---- gp_gemm_split256
    ("gp_gemm_split256", dict(scratch_bytes=4096), "scratch too small", None),
    ("gp_gemm_split256", dict(J=2048, ld_act=2048, ldd=2048, ldr=2048), "with >= 256 tiles", None),
    ("gp_gemm_split256", dict(whi=P[1] + 8), "null / misaligned operand", None),
    ("gp_gemm_split256", dict(I=131072), "output too large", None),
    ("gp_gemm_split256", dict(ld_act=16638), "ld_act=16638 is below the activation extent 16640", NEW),
    ("gp_gemm_split256", dict(ldd=16636), "ldd=16636 is below J=16640", NEW),
    ("gp_gemm_split256", dict(epilogue=2, bias=0), "epilogue 2 needs a bias", NEW),
    ("gp_gemm_split256", dict(scale=0), "epilogue 3 needs scale and residual", NEW),
    ("gp_gemm_split256", dict(residual=0), "epilogue 3 needs scale and residual", NEW),
    ("gp_gemm_split256", dict(ldr=16636), "ldr=16636 is below J=16640", NEW),
    ("gp_gemm_split256", dict(epilogue=9), "epilogue 9 is not built", NEW),   # stood in the launcher, behind the scratch reset (a HIP call)
    # ---- gp_gemm_planes256_scaled
    ("gp_gemm_planes256_scaled", dict(scratch=0), "scratch too small", None),
    ("gp_gemm_planes256_scaled", dict(I=1000), "must be multiples of 256", None),
    ("gp_gemm_planes256_scaled", dict(J_valid=16641), "must be multiples of 256", None),
    ("gp_gemm_planes256_scaled", dict(I=16384, J_valid=16639), "must be multiples of 256", None),   # 512 x 8 strip fragments: the 12-bit counter
    ("gp_gemm_planes256_scaled", dict(b_lo=0), "null / misaligned operand", None),
    ("gp_gemm_planes256_scaled", dict(I=1048576, K=1024, J_valid=16640), "operand planes too large", None),
    ("gp_gemm_planes256_scaled", dict(epilogue=9), "epilogue 9 is not built", NEW),                  # as gp_gemm_split256's
    ("gp_gemm_planes256_scaled", dict(bias=0), "epilogue 3 needs a bias", NEW),
    ("gp_gemm_planes256_scaled", dict(bias=P[7] + 4), "bias must be 16-byte aligned", NEW),
    ("gp_gemm_planes256_scaled", dict(D=0), "bad f32 output", None),
    ("gp_gemm_planes256_scaled", dict(ldd=16642), "bad f32 output", None),
    ("gp_gemm_planes256_scaled", dict(residual=P[9] + 8), "bad f32 output", None),
    ("gp_gemm_planes256_scaled", dict(ldd=16636), "ldd=16636 is below J=16640", NEW),
    ("gp_gemm_planes256_scaled", dict(scale=0), "epilogue 3 needs a 16-byte aligned scale and a residual", NEW),
    ("gp_gemm_planes256_scaled", dict(residual=0), "epilogue 3 needs a 16-byte aligned scale and a residual", NEW),
    ("gp_gemm_planes256_scaled", dict(ldr=16636), "ldr=16636 is below J=16640", NEW),
    ("gp_gemm_planes256_scaled", dict(plane_scale=16.0), "a plane scale other than 8 needs epilogue 6 or 7", None),
    # the first sizes beyond the 0x7ffffff0 bytes the tile epilogues' buffer resources address (the largest accepted: test_gpu_gemm_layout.py)
    ("gp_gemm_planes256_scaled", dict(J=524288, J_valid=524288, ldd=524288, ldr=524288, K=32), "D of I=1024 rows x ldd=524288 ends beyond", NEW),
    ("gp_gemm_planes256_scaled", dict(J=524032, J_valid=524032, ldd=524032, ldr=524544, K=32), "residual of I=1024 rows x ldr=524544 ends beyond", NEW),
    ("gp_gemm_planes256_scaled", dict(PLANES7, bias=0), "epilogue 7 needs a bias", None),             # stood as "bad plane output"
    ("gp_gemm_planes256_scaled", dict(PLANES7, out_lo=0), "bad plane output", None),
    ("gp_gemm_planes256_scaled", dict(PLANES7, ldo=1028), "plane output rows must be 16-byte aligned", None),
    ("gp_gemm_planes256_scaled", dict(PLANES7, ldo=1016), "ldo=1016 is below I=1024", NEW),
    ("gp_gemm_planes256_scaled", dict(PLANES7, I=4096, ldo=4096, J=262144, J_valid=262144, K=32), "output planes of J=262144 rows x ldo=4096 end beyond", NEW),
]


def invoke(lib, entry, changes):
    names, has_scratch, base = ENTRIES[entry]
    unknown = set(changes) - set(names) - {"scratch", "scratch_bytes"}
    assert not unknown, unknown
    args = dict(base, **changes)
    tail = []
    if has_scratch:
        tail = [args.get("scratch", P[11]), args.get("scratch_bytes", getattr(lib, WORKSPACE[entry])())]
    return getattr(lib, entry)(*[args[n] for n in names], *tail, None)   # stream = NULL


@pytest.fixture(params=["product", "probe"])
def library(request):
    if request.param == "product":
        yield _lib.lib()
    else:
        with _lib.probe_library() as lib:
            yield lib


@pytest.mark.parametrize("entry,changes,message,new", CASES,
                         ids=[f"{i:02d}-{e[3:]}-{m[:36].strip().replace(' ', '_')}" for i, (e, c, m, n) in enumerate(CASES)])
def test_refused_with_the_requirement_named(library, entry, changes, message, new):
    rc = invoke(library, entry, changes)
    said = library.gp_last_error().decode()
    assert rc == -1 and message in said, f"{entry}({changes}) -> {rc}: {said!r}"


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_base_arguments_pass_every_guard(library, entry):
    """The cases above prove a guard only if the call they start from is accepted: it gets as far as a HIP call, which fails without a device."""
    variants = [{}]
    if entry == "gp_gemm_planes256_scaled":
        variants += [PLANES7,
                     # the largest sizes the byte-range guards accept (multiples of 256)
                     dict(J=524032, J_valid=524032, ldd=524032, ldr=524032, K=32),
                     dict(PLANES7, I=4096, ldo=4096, J=261888, J_valid=261888, K=32)]
    for changes in variants:
        rc = invoke(library, entry, changes)
        assert rc == -2, f"{entry}({changes}) -> {rc}: {library.gp_last_error().decode()!r}"
