"""GPU: a call that passes tensors and numbers directly (the arguments converted from the header's prototype, gigapose_amd/_lib.py)
launches what the same call with explicit ctypes values launches, on the product library and on a front-end library; a tensor the
kernels cannot take is refused by the parameter's name before the library is entered."""
import ctypes

import pytest
import torch

from gigapose_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), what


def test_topk_plain_arguments_equal_explicit_ctypes():
    B, N, k = 2, 5, 3
    sim = torch.tensor([[0.25, 0.75, -1.0, 0.75, 0.5], [0.0, -0.5, 3.0, 1e-30, -2.0]], dtype=torch.float32, device=DEV)   # row 0 holds a tie
    out = []
    for style in ("plain", "explicit"):
        ids = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
        scores = torch.full((B, k), float("nan"), dtype=torch.float32, device=DEV)
        if style == "plain":
            _lib.call("gp_topk", sim, B, N, k, ids, scores, _lib.stream_ptr())
        else:
            _lib.call("gp_topk", ctypes.c_void_p(sim.data_ptr()), ctypes.c_int(B), ctypes.c_int(N), ctypes.c_int(k), ctypes.c_void_p(ids.data_ptr()),
                      ctypes.c_void_p(scores.data_ptr()), _lib.stream_ptr())
        out.append((ids, scores))
    assert_same_bits(out[0][0], out[1][0], "ids")
    assert_same_bits(out[0][1], out[1][1], "scores")
    assert out[0][0].tolist() == [[1, 3, 4], [2, 3, 0]]     # ties: the lower index first (include/gigapose_hip.h)
    assert_same_bits(out[0][1], torch.gather(sim, 1, out[0][0].long()), "scores are the selected values")


def test_root_long_long_count_through_a_side_library():
    from gigapose_amd import distances

    x = torch.tensor([2.0, 3.0, 4503599627370497.0], dtype=torch.float64, device=DEV)
    plain, explicit = torch.full_like(x, -1.0), torch.full_like(x, -2.0)
    distances._dist.call("gpd_root", x, x.shape[0], plain, _lib.stream_ptr())
    distances._dist.call("gpd_root", _lib.ptr(x), ctypes.c_longlong(3), _lib.ptr(explicit), _lib.stream_ptr())
    assert_same_bits(plain, explicit, "gpd_root")
    assert_same_bits(plain, torch.sqrt(x.cpu()), "gpd_root is the correctly rounded root")
    assert_same_bits(distances.roots(x), plain, "distances.roots")


def test_a_strided_tensor_is_refused_by_name_before_the_library_is_entered():
    lib = _lib.lib()
    with pytest.raises(_lib.GigaPoseHipError, match="gp_topk failed"):
        _lib.call("gp_topk", None, 1, 3, 5, None, None, None)
    before = lib.gp_last_error()
    t = torch.zeros(2, 10, dtype=torch.float32, device=DEV)[:, ::2]
    assert not t.is_contiguous()
    ids = torch.full((2, 3), -7, dtype=torch.int32, device=DEV)
    scores = torch.zeros(2, 3, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.GigaPoseHipError, match=r"gp_topk: argument 1 \(pointer sim_avg\): non-contiguous"):
        _lib.call("gp_topk", t, 2, 5, 3, ids, scores, _lib.stream_ptr())
    with pytest.raises(_lib.GigaPoseHipError, match=r"gp_topk: argument 6 \(pointer scores\): non-contiguous"):
        _lib.call("gp_topk", t.contiguous(), 2, 5, 3, ids, t, _lib.stream_ptr())
    with pytest.raises(_lib.GigaPoseHipError, match="ptr_table: entry 1: non-contiguous"):
        _lib.ptr_table([ids, t])
    with pytest.raises(_lib.GigaPoseHipError, match="non-contiguous"):
        _lib.ptr(t)
    torch.cuda.synchronize()
    assert lib.gp_last_error() == before and (ids == -7).all()      # nothing ran
    table = _lib.ptr_table([ids, scores])
    assert [table[0], table[1]] == [ids.data_ptr(), scores.data_ptr()]
