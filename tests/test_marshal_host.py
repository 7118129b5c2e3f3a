"""CPU: _lib.marshal converts the arguments of a call by the kinds its prototype declares.  The prototypes come from a header string, so
no library and no device is needed; the last tests go through the product library and libgigapose_eval.so, which load without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from gigapose_amd import _lib

HEADER = """
int f(const float* src, int count, long long total, size_t bytes, float gain, double eps, void* stream);
"""
RESTYPE, ARGTYPES, NAMES = _lib._parse(HEADER)["f"]
GOOD = (None, 1, 2, 3, 0.5, 0.25, None)
POS = {"src": 0, "count": 1, "total": 2, "bytes": 3, "gain": 4, "eps": 5, "stream": 6}
KIND = {"src": "pointer", "count": "int", "total": "long long", "bytes": "size_t", "gain": "float", "eps": "double", "stream": "pointer"}


def marshal_one(param, value):
    args = list(GOOD)
    args[POS[param]] = value
    return _lib.marshal("f", ARGTYPES, NAMES, args)[POS[param]]


def refused(param, value, error):
    """The error names the function, the 1-based position, the parameter and its kind."""
    with pytest.raises(error) as e:
        marshal_one(param, value)
    msg = str(e.value)
    assert "f: argument %d (%s %s)" % (POS[param] + 1, KIND[param], param) in msg, msg
    return msg


def test_the_internal_parse_keeps_the_names_and_the_public_one_its_shape():
    assert NAMES == ["src", "count", "total", "bytes", "gain", "eps", "stream"]
    assert ARGTYPES == [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.c_void_p]
    assert _lib.parse_prototypes(HEADER) == {"f": (RESTYPE, ARGTYPES)}
    assert _lib._parse("int g(const float* const* w, const int *n, int k);")["g"][2] == ["w", "n", "k"]


@pytest.mark.parametrize("param", ["count", "total", "bytes"])
def test_integer_kinds_take_python_and_numpy_integers_and_bool(param):
    for v in (7, True, np.int32(7), np.int64(7), np.uint8(7)):
        out = marshal_one(param, v)
        assert type(out) is int and out == int(v)
        assert ARGTYPES[POS[param]](out).value == int(v)   # what ctypes makes of it


def test_integer_ranges_are_the_declared_kinds():
    for param, lo, hi in (("count", -2 ** 31, 2 ** 31 - 1), ("total", -2 ** 63, 2 ** 63 - 1), ("bytes", 0, 2 ** 64 - 1)):
        assert marshal_one(param, lo) == lo and marshal_one(param, hi) == hi
        assert ARGTYPES[POS[param]](lo).value == lo and ARGTYPES[POS[param]](hi).value == hi   # nothing wraps inside the range
        for bad in (lo - 1, hi + 1):
            assert str(bad) in refused(param, bad, OverflowError)
    refused("count", 2 ** 31, OverflowError)
    refused("count", -2 ** 31 - 1, OverflowError)
    refused("bytes", -1, OverflowError)
    refused("bytes", 2 ** 64, OverflowError)
    refused("total", 2 ** 63, OverflowError)
    refused("count", np.int64(2 ** 31), OverflowError)


@pytest.mark.parametrize("param", ["count", "total", "bytes"])
def test_integer_kinds_refuse_what_is_no_integer(param):
    for v in (3.0, 3.9, np.float32(3), "3", None, [3]):
        refused(param, v, TypeError)


class Unreadable(torch.Tensor):
    """A tensor whose value cannot be read: reading it would be the hidden synchronisation."""

    def _no(self, *a, **k):
        raise AssertionError("the tensor was read")

    __index__ = __int__ = __float__ = __bool__ = item = tolist = _no


@pytest.mark.parametrize("param", ["count", "total", "bytes", "gain", "eps"])
def test_a_tensor_for_a_scalar_is_refused_unread(param):
    t = torch.tensor(3).as_subclass(Unreadable)
    with pytest.raises(AssertionError):
        t.item()
    refused(param, t, TypeError)
    refused(param, torch.tensor(3), TypeError)
    refused(param, torch.tensor(3.0), TypeError)


def test_a_host_tensor_for_a_pointer_is_refused_by_name():
    for param in ("src", "stream"):
        msg = refused(param, torch.zeros(4), _lib.GigaPoseHipError)
        assert "need tensors on the GPU (no CPU fallback)" in msg
    with pytest.raises(_lib.GigaPoseHipError, match="on the GPU"):
        _lib.ptr(torch.zeros(4))
    with pytest.raises(_lib.GigaPoseHipError, match="ptr_table: entry 0.*on the GPU"):
        _lib.ptr_table([torch.zeros(1), torch.zeros(1)])


def test_none_is_the_null_pointer():
    seen = []
    probe = ctypes.CFUNCTYPE(ctypes.c_int, *ARGTYPES)(lambda *a: seen.append(a) or 0)
    assert probe(*_lib.marshal("f", ARGTYPES, NAMES, GOOD)) == 0
    assert seen[0][0] is None and seen[0][6] is None and seen[0][1:6] == (1, 2, 3, 0.5, 0.25)   # ctypes hands a callback NULL as None
    assert _lib.ptr(None).value is None
    table = _lib.ptr_table([])
    assert len(table) == 1 and table[0] is None


def test_ctypes_instances_pass_by_identity():
    n, arr = ctypes.c_int(4), (ctypes.c_float * 3)(1, 2, 3)
    args = (arr, n, ctypes.c_longlong(5), ctypes.c_size_t(6), ctypes.c_float(1.5), ctypes.c_double(2.5), ctypes.byref(n))
    out = _lib.marshal("f", ARGTYPES, NAMES, args)
    assert all(a is b for a, b in zip(out, args))
    wrong = (ctypes.c_float(1.0), ctypes.c_float(1.0), ctypes.c_int(5), ctypes.c_int(6), ctypes.c_int(1), ctypes.c_int(2), ctypes.c_void_p(0))
    out = _lib.marshal("f", ARGTYPES, NAMES, wrong)     # a ctypes value of the wrong kind is ctypes' to refuse (ArgumentError, test_cabi.py)
    assert all(a is b for a, b in zip(out, wrong))
    for old in (_lib.i(3), _lib.f(3), _lib.d(3), _lib.ptr(None)):
        assert marshal_one("count", old) is old
    assert marshal_one("src", 1234) == 1234           # an address as an integer: as before


@pytest.mark.parametrize("param", ["gain", "eps"])
def test_real_kinds_take_real_numbers(param):
    for v in (1, 1.5, np.float64(1.5), np.float32(1.5), np.int32(2), True):
        out = marshal_one(param, v)
        assert type(out) is float and out == float(v)
    for v in ("1.5", b"1", None, 1j, torch.tensor(1.5), [1.5]):
        refused(param, v, TypeError)


def test_argument_count():
    with pytest.raises(TypeError, match=r"^f takes 7 arguments \(include/\), got 6$"):
        _lib.marshal("f", ARGTYPES, NAMES, GOOD[:-1])
    with pytest.raises(TypeError, match=r"^f takes 7 arguments \(include/\), got 8$"):
        _lib.marshal("f", ARGTYPES, NAMES, GOOD + (None,))


def test_plain_arguments_reach_the_product_library():
    lib = _lib.lib()
    with pytest.raises(_lib.GigaPoseHipError, match=r"gp_topk failed \(rc=-1\)"):
        _lib.call("gp_topk", None, 1, 3, 5, None, None, None)
    before = lib.gp_last_error()
    with pytest.raises(OverflowError, match=r"gp_topk: argument 3 \(int N\)"):
        _lib.call("gp_topk", None, 1, 2 ** 31, 5, None, None, None)
    with pytest.raises(TypeError, match=r"gp_topk: argument 2 \(int B\)"):
        _lib.call("gp_topk", None, 1.0, 3, 5, None, None, None)
    with pytest.raises(_lib.GigaPoseHipError, match=r"gp_topk: argument 1 \(pointer sim_avg\).*on the GPU"):
        _lib.call("gp_topk", torch.zeros(1, 3), 1, 3, 1, None, None, None)
    with pytest.raises(TypeError, match="gp_topk takes 7 arguments"):
        _lib.call("gp_topk", None, 1, 3, 5, None, None)
    assert lib.gp_last_error() == before               # refused before the library was entered


def test_sizes_come_back_whole_from_plain_integers():
    side = _lib.SideLibrary("libgigapose_eval.so", "gpe")
    want = 65535 * (2 ** 31 - 1) * 14 * 8
    assert side.lib().gpe_pose_workspace_bytes(65535, 2 ** 31 - 1) == want
    assert side.value("gpe_pose_workspace_bytes", 65535, 2 ** 31 - 1) == want
    with pytest.raises(OverflowError, match=r"gpe_pose_workspace_bytes: argument 2 \(int S\)"):
        side.value("gpe_pose_workspace_bytes", 65535, 2 ** 31)
