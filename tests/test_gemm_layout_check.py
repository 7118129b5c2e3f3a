"""CPU: gigapose_testing.gemm_layout.check accepts a numpy stand-in of a laid-out GEMM launch and rejects six subtly wrong ones -- the
mistakes tests/test_gpu_gemm_layout.py exists to find in the HIP epilogues."""
import numpy as np
import pytest
import torch

from gigapose_testing import gemm_layout as gl

I, J, K = 32, 48, 8
LDA, LDB, LDD, LDR, BASE = I + 12, J + 4, J + 8, J + 4, 4      # the offsets of the GPU cases, at toy size
A0, B0 = 4, 4                                                  # operand windows start 4 columns into their arrays
LDO, OFF, J_VALID = 3 * I, 2 * I, 40                           # plane output: the v launch's columns of a q | k | v row; rows < 64 are owned


def operands():
    rs = np.random.RandomState(3)
    A, B = rs.standard_normal((K, I)).astype(np.float32), rs.standard_normal((K, J)).astype(np.float32)
    bias, scale = rs.standard_normal(I).astype(np.float32), rs.standard_normal(I).astype(np.float32)
    res = rs.standard_normal((I, J)).astype(np.float32)
    return A, B, bias, scale, res


def epilogue3(Aw, Bw, bias, scale, resw):
    return (resw + scale[:, None] * (Aw.T @ Bw + bias[:, None])).astype(np.float32)


def f32_launch(fault=None, alias=False):
    """Epilogue 3 into D at BASE of a sentinel-filled buffer with stride LDD, operands and residual as windows; returns check's arguments."""
    A, B, bias, scale, res = operands()
    tight = epilogue3(A, B, bias, scale, res)
    Aw, Bw = gl.embed(torch.from_numpy(A), LDA, A0)[0].numpy(), gl.embed(torch.from_numpy(B), LDB, B0)[0].numpy()
    flat = gl.filled(BASE + I * LDD + 8, gl.F32_SENTINEL, torch.float32, "cpu").numpy()
    D = flat[BASE:BASE + I * LDD].reshape(I, LDD)
    if alias:
        D[:, :J] = res
        resbuf, ldr = D, LDD
    else:
        resbuf, ldr = gl.embed(torch.from_numpy(res), LDR)[0].numpy()[:I], LDR
    before = resbuf.copy()
    b0 = B0 - (1 if fault == "read one column outside" else 0)
    rld = LDD if fault == "residual read with ldd" else ldr
    r = np.lib.stride_tricks.as_strided(resbuf.reshape(-1), (I, J), (4 * rld, 4)) if rld * (I - 1) + J <= resbuf.size else None
    if r is None:   # ldd > ldr: the wrong stride runs off the residual buffer; a kernel would read whatever lies there
        pad = np.concatenate([resbuf.reshape(-1), np.zeros(rld * I, np.float32)])
        r = np.lib.stride_tricks.as_strided(pad, (I, J), (4 * rld, 4))
    out = epilogue3(Aw[:K, A0:A0 + I], Bw[:K, b0:b0 + J], bias, scale, r.copy())
    if fault == "tight stride":
        flat[BASE:BASE + I * J] = out.reshape(-1)
    else:
        D[:, :J] = out
    if fault == "one vector past":
        D[:, J:J + 4] = out[:, -4:]
    if fault == "writes the residual":
        resbuf[:I, :J] = out
    owned = [(BASE, LDD, I, J, torch.from_numpy(tight))]
    residual = None if alias else (torch.from_numpy(resbuf), torch.from_numpy(before))
    return torch.from_numpy(flat), gl.F32_SENTINEL, owned, "D", residual


def plane_launch(fault=None):
    """Epilogue 7's hi plane O[j][OFF + i] = f16(acc + bias[i]) for the 64 = round_up(J_VALID, 32) owned rows of a [J + 16][LDO] buffer."""
    A, B, bias, _, _ = operands()
    rows = (J_VALID + 31) // 32 * 32
    Bp = np.concatenate([B, B[:, :rows - J]], 1)                 # rows J_VALID .. 63 carry data too (the strip computes whole fragments)
    tight = (Bp.T @ A + bias[None, :]).astype(np.float16)
    flat = gl.filled((rows + 16) * LDO, gl.F16_SENTINEL_HI, torch.float16, "cpu").numpy()
    O = flat.reshape(rows + 16, LDO)
    if fault == "tight stride":
        flat[OFF:OFF + rows * I] = tight.reshape(-1)
    else:
        O[:rows, OFF:OFF + I] = tight
    if fault == "rows beyond the strip cleared":
        O[rows:, OFF:OFF + I] = 0
    if fault == "one vector past":
        O[:rows, OFF - 8:OFF] = tight[:, :8]
    return torch.from_numpy(flat), gl.F16_SENTINEL_HI, [(OFF, LDO, rows, I, torch.from_numpy(tight))], "out_hi", None


def test_a_correct_launch_passes():
    for args in (f32_launch(), f32_launch(alias=True), plane_launch()):
        gl.check(*args[:3], what=args[3], residual=args[4])


@pytest.mark.parametrize("launch,fault,says", [
    (f32_launch, "tight stride", "differs from the tight launch"),                 # a store with the tight stride in place of ldd
    (plane_launch, "tight stride", "differs from the tight launch"),               # ... in place of ldo
    (f32_launch, "one vector past", "outside every owned window was written"),     # a store one vector past the owned columns
    (plane_launch, "one vector past", "outside every owned window was written"),   # ... into the q | k launch's columns
    (f32_launch, "residual read with ldd", "holds a NaN|differs from the tight"),  # ldd in place of ldr (runs into the residual's NaN pad columns)
    (f32_launch, "writes the residual", "the residual buffer was written"),        # an epilogue that writes the residual buffer
    (f32_launch, "read one column outside", "holds a NaN"),                        # a read one column outside the operand window
    (plane_launch, "rows beyond the strip cleared", "outside every owned window was written"),   # rows beyond the strip cleared to zero
])
def test_a_wrong_launch_is_rejected(launch, fault, says):
    flat, sentinel, owned, what, residual = launch(fault)
    with pytest.raises(AssertionError, match=says):
        gl.check(flat, sentinel, owned, what=what, residual=residual)


def test_a_write_before_the_base_is_rejected():
    flat, sentinel, owned, what, residual = f32_launch()
    flat[BASE - 1] = 0.0
    with pytest.raises(AssertionError, match="1 before its base"):
        gl.check(flat, sentinel, owned, what=what, residual=residual)
