"""What a GEMM launch may touch, given its leading dimensions and base pointers (tests/test_gpu_gemm_layout.py; its own test with wrong
stand-ins: tests/test_gemm_layout_check.py).

A laid-out launch -- operands as windows of wider arrays, an output with ld > width or at an offset into its buffer, a residual that is not
the output -- runs the same schedule as the tight launch of the same shape (ld == width, base == buffer), so its owned window must equal
the tight result bit for bit; the tight launches are the ones held to float64 and the oracle elsewhere.  Everything around the window
shows what else was touched:
  * operands are embedded in arrays filled with NaN (embed): a read outside the window turns an output into NaN;
  * output buffers are filled with a sentinel (filled): a store outside the window overwrites it;
  * a residual that is not the output must come back unchanged.
Tensors on any device; comparisons are on the bits (a -0.0 for a +0.0 is a difference, a sentinel NaN would compare equal to itself)."""
import dataclasses

import torch

F32_SENTINEL = -7654321.5            # exact in f32; no case produces a whole vector of it
F16_SENTINEL_HI, F16_SENTINEL_LO = 1234.0, -0.40625   # exact f16 values (the pair tests/test_gpu_attention_split.py uses)

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16}


def embed(x, ld, col0=0, rows_after=1):
    """x (rows, cols) as the window [0:rows, col0:col0 + cols] of a NaN-filled (rows + rows_after, ld) array: (whole array, window view)."""
    rows, cols = x.shape
    assert col0 + cols <= ld
    whole = torch.full((rows + rows_after, ld), float("nan"), dtype=x.dtype, device=x.device)
    whole[:rows, col0:col0 + cols] = x
    return whole, whole[:rows, col0:col0 + cols]


def filled(numel, sentinel, dtype, device):
    """A flat output buffer nobody has written."""
    return torch.full((numel,), sentinel, dtype=dtype, device=device)


@dataclasses.dataclass
class Layout:
    """How a test helper lays a launch out; every default is the tight value the helpers use without one."""
    a_ld: int = None      # first f32 operand (A, or the split GEMMs' activation): leading dimension ...
    a_col: int = 0        # ... and the column its window starts at (keep 16-byte alignment: multiples of 4)
    b_ld: int = None      # second f32 operand (gp_gemm_kmajor's B)
    b_col: int = 0
    d_ld: int = None      # f32 output
    d_base: int = 0       # elements between the buffer's start and D
    r_ld: int = None      # epilogue 3: None = the residual is D itself, else a buffer of its own with this leading dimension
    o_ld: int = None      # plane outputs (epilogues 6 / 7): row stride, first column, and the (hi, lo) flat buffers to write into
    o_col: int = 0        # (None: sentinel-filled ones of their own)
    o_bufs: tuple = None


def place_output(L, I, J, epi, res, device):
    """The f32 side of a laid-out launch: (flat sentinel-filled buffer, D view, residual view or None, ldr, (residual array, its copy) or
    None).  res (I, J) on the device, used by epilogue 3: copied into D when the launch is in place, embedded in NaN when it is not."""
    ldd = L.d_ld or J
    flat = filled(L.d_base + I * ldd + 8, F32_SENTINEL, torch.float32, device)
    D = window(flat, L.d_base, ldd, I, J)
    if epi != 3:
        return flat, D, None, ldd, None
    if L.r_ld is None:
        D.copy_(res)
        return flat, D, D, ldd, None
    whole, win = embed(res, L.r_ld)
    return flat, D, win, L.r_ld, (whole, whole.clone())


def place_planes(L, I, rows, device):
    """The plane side: (hi flat, lo flat, ldo), sentinel-filled with 32 spare rows unless the layout brings its buffers."""
    ldo = L.o_ld or I
    if L.o_bufs is not None:
        return L.o_bufs[0], L.o_bufs[1], ldo
    return (filled((rows + 32) * ldo, F16_SENTINEL_HI, torch.float16, device), filled((rows + 32) * ldo, F16_SENTINEL_LO, torch.float16, device), ldo)


def window(flat, base, ld, rows, cols):
    """The (rows, cols) view of a flat buffer a launch with this base offset (elements) and leading dimension owns."""
    assert base >= 0 and cols <= ld and base + (rows - 1) * ld + cols <= flat.numel()
    return flat.as_strided((rows, cols), (ld, 1), base)


def check(flat, sentinel, owned, what="output", residual=None):
    """flat: the whole output buffer after the launch(es), filled(.., sentinel) before; owned: [(base, ld, rows, cols, tight)], the windows
    the launches own and what the tight launch of each left; residual: (after, before) of a residual that is not the output, or None.
    Raises AssertionError naming the first thing found:
      * an owned window is not the tight result bit for bit, or holds a NaN (something outside an operand window was read);
      * an element outside every owned window no longer holds the sentinel: pad columns between a row's width and its stride, columns
        of a plane row outside the launch's own, rows below the last owned one, anything before the base offset;
      * the residual changed."""
    bits = _BITS[flat.dtype]
    left = flat.clone()
    sent = torch.tensor(sentinel, dtype=flat.dtype, device=flat.device)
    for k, (base, ld, rows, cols, tight) in enumerate(owned):
        win = window(flat, base, ld, rows, cols)
        assert tuple(tight.shape) == (rows, cols) and tight.dtype == flat.dtype
        nan = torch.isnan(win)
        if bool(nan.any()):
            r, c = (int(v) for v in nan.nonzero()[0])
            raise AssertionError(f"{what}: window {k} holds a NaN at ({r}, {c}) ({int(nan.sum())} in all): something outside an operand window was read")
        diff = win.contiguous().view(bits) != tight.to(flat.device).contiguous().view(bits)
        if bool(diff.any()):
            r, c = (int(v) for v in diff.nonzero()[0])
            raise AssertionError(f"{what}: window {k} differs from the tight launch at ({r}, {c}): {float(win[r, c])!r} for {float(tight[r, c])!r} "
                                 f"({int(diff.sum())} of {rows * cols} elements)")
        window(left, base, ld, rows, cols).copy_(sent)
    touched = left.view(bits) != sent.view(bits)
    if bool(touched.any()):
        at = int(touched.nonzero()[0])
        where = "; ".join(f"window {k}: row {(at - base) // ld}, column {(at - base) % ld} of stride {ld}" if at >= base else f"window {k}: {base - at} before its base"
                          for k, (base, ld, rows, cols, tight) in enumerate(owned))
        raise AssertionError(f"{what}: element {at} outside every owned window was written ({float(flat[at])!r} for the sentinel; {int(touched.sum())} in all) -- {where}")
    if residual is not None:
        after, before = residual
        changed = after.contiguous().view(_BITS[after.dtype]) != before.to(after.device).contiguous().view(_BITS[before.dtype])
        if bool(changed.any()):
            raise AssertionError(f"{what}: the residual buffer was written ({int(changed.sum())} elements changed)")
