"""CPU: the nine libraries load (without a GPU), export exactly what their headers declare, and carry the headers' types in ctypes.

include/gigapose_hip.h        <->  gigapose_amd/libgigapose_hip.so         (the product: at most 45 entry points, no A/B switches)
include/gigapose_hip_probe.h  <->  gigapose_amd/libgigapose_hip_probe.so   (the same sources with -DGP_PROBES: + hooks / traced builds)
include/gigapose_<name>.h     <->  gigapose_amd/libgigapose_<name>.so      (the seven front-end libraries)
The declared names and types come from the package's own parser (_lib.parse_prototypes): what the tests see is what the bindings use."""
import ctypes
import subprocess

import pytest

from gigapose_amd import _lib

SIDE = {"ingest": "gpi", "rlestr": "gps", "onboard": "gpo", "render": "gpr", "texture": "gpt", "eval": "gpe", "dist": "gpd"}


def declared_symbols(*headers):
    return sorted(_lib.declared(*headers))


def exported_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if " T gp" in ln})


def side_library(name):
    return _lib.SideLibrary(f"libgigapose_{name}.so", SIDE[name])   # a handle of its own: nothing but the loader has touched it


def assert_typed(handle, protos):
    for name, (restype, argtypes) in protos.items():
        fn = getattr(handle, name)
        assert fn.restype is restype, f"{name}: restype {fn.restype}, declared {restype}"
        assert list(fn.argtypes) == argtypes, f"{name}: argtypes {fn.argtypes}, declared {argtypes}"


def test_product_library_exports_exactly_the_product_header():
    lib = _lib.lib()
    names = declared_symbols("gigapose_hip.h")
    assert 7 <= len(names) <= 45, f"{len(names)} entry points in the product header (the bar is 45)"
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gigapose_hip.h but not exported"
    assert exported_symbols(_lib.LIB_PATH) == names, "the product library exports something its header does not declare (or the reverse)"
    assert not [n for n in names if "_set_" in n and n != "gp_set_status_buffer"], "an A/B switch in the product interface"
    assert lib.gp_abi_version() >= 2


def test_probe_library_adds_the_probe_header_and_nothing_undeclared():
    product, probe = declared_symbols("gigapose_hip.h"), declared_symbols("gigapose_hip_probe.h")
    assert not set(product) & set(probe)
    assert exported_symbols(_lib.PROBE_LIB_PATH) == sorted(product + probe)
    with _lib.probe_library() as lib:
        for n in probe:
            assert hasattr(lib, n)
        assert _lib.lib() is lib
    assert _lib.lib() is not lib


@pytest.mark.parametrize("name", sorted(SIDE))
def test_side_library_exports_exactly_its_header_with_its_types(name):
    side = side_library(name)
    protos = _lib.declared(side.header)
    assert side.header == f"gigapose_{name}.h" and all(n.startswith(SIDE[name] + "_") for n in protos)
    assert exported_symbols(side.path) == sorted(protos)
    assert_typed(side.lib(), protos)


def test_every_declared_function_carries_its_header_types():
    product = _lib.declared("gigapose_hip.h")
    assert_typed(_lib.lib(), product)
    with _lib.probe_library() as lib:
        probe = _lib.declared("gigapose_hip_probe.h")
        assert_typed(lib, {**product, **probe})
        assert lib.gp_vit_set_ln_live.restype is None and lib.gp_gemm_set_streamk.restype is None     # void
    lib = _lib.lib()
    assert lib.gp_prof_begin.restype is None and lib.gp_last_error.restype is ctypes.c_char_p
    # sizes: an int restype would truncate them to 32 bits without an error
    for fn in (lib.gp_vit_workspace_bytes, lib.gp_conv2d_planes_workspace_bytes, lib.gp_ist_workspace_bytes,
               side_library("render").lib().gpr_raster_workspace_bytes, side_library("eval").lib().gpe_pose_workspace_bytes,
               side_library("texture").lib().gpt_mip_texels):
        assert fn.restype is ctypes.c_size_t, fn.__name__
    assert side_library("eval").lib().gpe_pose_workspace_bytes(65535, 2 ** 31 - 1) == 65535 * (2 ** 31 - 1) * 14 * 8
    assert lib.gp_split256_weights.argtypes[1] is ctypes.c_size_t and lib.gp_topk.argtypes[0] is ctypes.c_void_p


def test_argument_validation_needs_no_gpu():
    lib = _lib.lib()
    rc = lib.gp_topk(None, 1, 3, 5, None, None, None)
    assert rc == -1 and b"gp_topk" in lib.gp_last_error()


def test_wrong_calls_fail_in_python():
    """Count and kind are checked against the header before the library is entered: its last error stays what it was."""
    lib = _lib.lib()
    assert lib.gp_topk(None, 1, 3, 5, None, None, None) == -1
    before = lib.gp_last_error()
    null, i = ctypes.c_void_p(0), _lib.i
    good = (null, i(1), i(3), i(5), null, null, null)
    with pytest.raises(TypeError, match="gp_topk takes 7 arguments"):
        _lib.call("gp_topk", *good, null)
    with pytest.raises(TypeError, match="gp_topk takes 7 arguments"):
        _lib.call("gp_topk", *good[:-1])
    with pytest.raises(ctypes.ArgumentError):   # size_t count
        _lib.call("gp_split256_weights", null, ctypes.c_int(4), null, null, null)
    with pytest.raises(ctypes.ArgumentError):   # a float for a pointer
        _lib.call("gp_topk", ctypes.c_float(1.0), *good[1:])
    with pytest.raises(TypeError, match="gpe_pose_workspace_bytes takes 2 arguments"):
        side_library("eval").call("gpe_pose_workspace_bytes", i(1))
    assert lib.gp_last_error() == before


def test_the_parser_rejects_what_it_cannot_read():
    ok = _lib.parse_prototypes('/* c */ #define X 1\nextern "C" {\nsize_t f(const float* const* w, size_t n, long long k, double d /* x */);\nvoid g(void);\n}')
    assert ok == {"f": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_double]), "g": (None, [])}
    for bad in ("int f(struct box b);",           # a struct by value
                "int f(unsigned n);",             # a scalar kind the headers do not use
                "int f(int);",                    # no parameter name
                "float f(int a);",                # a return kind the headers do not use
                "typedef int gp_t;",              # not a prototype
                "int f(int a); int f(int a);"):   # declared twice
        with pytest.raises(_lib.GigaPoseHipError):
            _lib.parse_prototypes(bad)


def test_a_missing_header_is_an_error():
    with pytest.raises(_lib.GigaPoseHipError, match="gigapose_nowhere.h not found"):
        _lib.declared("gigapose_nowhere.h")
