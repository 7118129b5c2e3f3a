"""ctypes binding of libgigapose_hip.so (C-ABI: include/gigapose_hip.h), and SideLibrary: the loader of the front-end libraries
(the fifteen of them: libgigapose_ingest / _rlestr / _onboard / _render / _texture / _eval / _dist / _refine / _verify / _maskfit / _shade / _gtinfo / _label / _coco / _appear.so; seventeen
libraries in all with the product library and its probe build), whose modules hold one instance each.

The product path has NO fallback: if the HIP library is missing or a call fails this module
raises.  torch must be imported first so the library binds to the HIP runtime torch already
loaded (same SONAME libamdhip64.so.7) and shares its streams and allocations.
"""
import ctypes
import operator
import os
import re

import numpy as np
import torch  # noqa: F401  (must precede the CDLL so both use one HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GIGAPOSE_LIB") or os.path.join(_HERE, "libgigapose_hip.so")   # GIGAPOSE_LIB: another build of the same sources (A/B of two commits, tools/)
PROBE_LIB_PATH = os.path.join(_HERE, "libgigapose_hip_probe.so")   # the same sources with -DGP_PROBES (include/gigapose_hip_probe.h)
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")   # the C headers: where every signature is stated (parse_prototypes)
_lib = None          # the library calls go to: the product library unless probe_library() is active
_product = None
_probe = None


class GigaPoseHipError(RuntimeError):
    pass


NUMERICS = ("split", "chain")


def default_numerics():
    """Numerics of the contraction kernels when nothing else is said: "split" -- every f32 operand as two
    f16 planes, 3 x f16 MFMA per k-block, f32 accumulate; f32-class accuracy (error vs float64 at or below a sequential f32
    chain's) at ~3x the speed -- is what the drop-in selects and what bench.py measures.  "chain" (env GIGAPOSE_NUMERICS=chain,
    `numerics: chain` in the model YAML, or model.set_numerics("chain")) is the verification mode: f32-input MFMA, every dot
    product the k-ordered fmaf chain the CPU oracle restates, bit-exact against it."""
    mode = os.environ.get("GIGAPOSE_NUMERICS", "split")
    if mode not in NUMERICS:
        raise ValueError(f"GIGAPOSE_NUMERICS must be one of {NUMERICS}, got {mode!r}")
    return mode


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}
_RANGES = {ctypes.c_int: ("int", -2 ** 31, 2 ** 31 - 1), ctypes.c_longlong: ("long long", -2 ** 63, 2 ** 63 - 1), ctypes.c_size_t: ("size_t", 0, 2 ** 64 - 1)}
_REALS = {ctypes.c_float: "float", ctypes.c_double: "double"}
_CTYPES = (ctypes.c_int.__mro__[-2], type(ctypes.byref(ctypes.c_int())))   # every ctypes instance, and what byref returns


def _parse(text):
    """parse_prototypes with the parameter names kept: {name: (restype, [argtypes], [parameter names])}."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    protos = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.*?) ?(\w+) ?\((.*)\)", stmt)
        ret = m and re.sub(r" ?\* ?", "*", m.group(1))
        params = m and ([] if m.group(3).strip() in ("", "void") else m.group(3).split(","))
        kinds = m and ["*" if "*" in p else " ".join(p.split()[:-1]) for p in params]   # a scalar is `type name`
        if not m or ret not in _RETURNS or m.group(2) in protos or any(k != "*" and k not in _SCALARS for k in kinds):
            raise GigaPoseHipError(f"cannot read the prototype `{stmt}`: expected `int|size_t|void|const char* name(params)`, each name once, "
                                   f"every parameter a pointer or a named {' | '.join(_SCALARS)}")
        protos[m.group(2)] = (_RETURNS[ret], [ctypes.c_void_p if k == "*" else _SCALARS[k] for k in kinds],
                              [re.search(r"\w*$", p.strip()).group() for p in params])
    return protos


def parse_prototypes(text):
    """The `ret name(params);` prototypes of a C header -> {name: (restype, [argtypes])}.  Reads what include/*.h use and is no C front end: comments,
    preprocessor lines and the extern "C" braces are dropped; a parameter is a pointer (-> c_void_p: None, an integer, a ctypes array or byref) or a named
    int, float, double, long long or size_t; a function returns int, size_t, void or const char*.  Anything else raises: a prototype is never skipped."""
    return {name: (restype, argtypes) for name, (restype, argtypes, _) in _parse(text).items()}


def _declared(*headers):
    protos = {}
    for path in (os.path.join(INCLUDE_DIR, h) for h in headers):
        if not os.path.exists(path):
            raise GigaPoseHipError(f"{path} not found: the ctypes signatures are read from the C headers beside the package (INTEGRATION.md section 2)")
        with open(path) as fh:
            protos.update(_parse(fh.read()))
    return protos


def declared(*headers):
    """The prototypes of include/<header>, ... together; a missing header is an error like a missing library."""
    return {name: (restype, argtypes) for name, (restype, argtypes, _) in _declared(*headers).items()}


def _address(t, where):
    """Device address of a contiguous GPU tensor; `where` names the call and the parameter."""
    if not t.is_cuda:
        raise GigaPoseHipError(f"{where}: gigapose_amd kernels need tensors on the GPU (no CPU fallback)")
    if not t.is_contiguous():
        raise GigaPoseHipError(f"{where}: non-contiguous tensor passed to a HIP kernel")
    return t.data_ptr()


def _converter(name, pos, pname, ctype):
    """What turns one argument of `name` into what ctypes takes for the declared kind.  A ctypes instance (c_void_p, an array, byref, c_int, ...) always
    passes unchanged: ctypes holds it against the argtypes.  A tensor is read only where a pointer is declared, so that no scalar synchronises the stream."""
    if ctype is ctypes.c_void_p:
        where = f"{name}: argument {pos} (pointer {pname})"

        def pointer(v):   # None is ctypes' NULL
            return _address(v, where) if isinstance(v, torch.Tensor) else v
        return pointer
    if ctype in _RANGES:
        kind, lo, hi = _RANGES[ctype]
        where = f"{name}: argument {pos} ({kind} {pname})"

        def integer(v):
            if type(v) is not int:
                if isinstance(v, _CTYPES):
                    return v
                if isinstance(v, torch.Tensor):
                    raise TypeError(f"{where} takes an integer, not a tensor: reading one on the device would synchronise the stream")
                try:
                    v = operator.index(v)
                except TypeError:
                    raise TypeError(f"{where} takes an integer, got {type(v).__name__}") from None
            if not lo <= v <= hi:
                raise OverflowError(f"{where}: {v} is outside [{lo}, {hi}]")
            return v
        return integer
    where = f"{name}: argument {pos} ({_REALS[ctype]} {pname})"

    def real(v):
        if type(v) is float or isinstance(v, _CTYPES):
            return v
        if isinstance(v, (torch.Tensor, str, bytes)):
            raise TypeError(f"{where} takes a real number, got {type(v).__name__}")
        try:
            return float(v)
        except (TypeError, ValueError):
            raise TypeError(f"{where} takes a real number, got {type(v).__name__}") from None
    return real


def converters(name, argtypes, names):
    """One converter per parameter of `name`: built once per function (_load), so that a call only applies them."""
    return tuple(_converter(name, pos, pname, ctype) for pos, (pname, ctype) in enumerate(zip(names, argtypes), 1))


def _convert(name, convs, args):
    if len(args) != len(convs):   # ctypes itself rejects too few arguments but lets extra ones through
        raise TypeError(f"{name} takes {len(convs)} arguments (include/), got {len(args)}")
    return [c(a) for c, a in zip(convs, args)]


def marshal(name, argtypes, names, args):
    """The arguments of one call as ctypes takes them, converted by the declared kinds (see _converter): tensors and None for pointers, Python and numpy
    integers in the declared range for int / long long / size_t, real numbers for float / double.  Needs no library: _load keeps the converters per function."""
    return tuple(_convert(name, converters(name, argtypes, names), args))


def _load(path, *headers, scope=" for the hot path"):
    """CDLL(path) with restype, argtypes and argument converters of every function the headers declare: a wrong argument kind is an error before the library is entered."""
    if not os.path.exists(path):
        raise GigaPoseHipError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               f"(there is deliberately no CPU / PyTorch fallback{scope})")
    h = ctypes.CDLL(path)
    h.gp_converters = {}
    for name, (restype, argtypes, names) in _declared(*headers).items():
        getattr(h, name).restype, getattr(h, name).argtypes = restype, argtypes
        h.gp_converters[name] = converters(name, argtypes, names)
    return h


def _invoke(h, name, args):
    fn = getattr(h, name)
    return fn(*_convert(name, h.gp_converters[name], args))


class SideLibrary:
    """A front-end library next to this file, exporting `<prefix>_*` as include/<its name>.h declares them: loaded on first use; a missing file is an error."""

    def __init__(self, file_name, prefix):
        self.path = os.path.join(_HERE, file_name)
        self.header = file_name[len("lib"):-len(".so")] + ".h"   # libgigapose_eval.so <-> include/gigapose_eval.h
        self.prefix = prefix
        self._handle = None

    def lib(self):
        if self._handle is None:
            self._handle = _load(self.path, self.header, scope="")
        return self._handle

    def call(self, name, *args):
        rc = _invoke(self.lib(), name, args)
        if rc != 0:
            raise GigaPoseHipError(f"{name} failed (rc={rc}): {getattr(self.lib(), self.prefix + '_last_error')().decode()}")

    def value(self, name, *args):
        """A function that returns no status (a size, a count, or nothing): its result, the arguments converted as call() converts them."""
        return _invoke(self.lib(), name, args)


def _expect(t, dtype, shape, who, what):
    """dtype (None: any), rank and fixed sizes of one tensor, or ValueError."""
    if (dtype is not None and t.dtype != dtype) or t.dim() != len(shape) or any(s is not None and s != g for s, g in zip(shape, t.shape)):
        want, got = tuple('*' if s is None else s for s in shape), tuple(t.shape)
        raise ValueError(f"{who}: expected {what} {want}, got {got}" if dtype is None else f"{who}: expected {what} {dtype} {want}, got {t.dtype} {got}")


def arg(t, dtype, shape, who, what):
    """Argument checks the front-end modules share.  Type, dtype, shape and layout of one argument (ValueError); on_gpu checks the devices once every argument has passed."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {what} must be a torch tensor, got {type(t).__name__}")
    _expect(t, dtype, shape, who, what)
    if not t.is_contiguous():
        raise ValueError(f"{who}: {what} is not contiguous")
    return t


def on_gpu(who, **tensors):
    for what, t in tensors.items():
        if not t.is_cuda:
            raise GigaPoseHipError(f"{who} needs {what} on the GPU (no CPU fallback)")


def checked(a, dtype, shape, who, what):
    """A numpy array or a tensor anywhere -> a tensor whose shape and kind of dtype are checked; upload moves it."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    _expect(t, None, shape, who, what)
    if t.dtype.is_floating_point != dtype.is_floating_point:
        raise ValueError(f"{who}: {what} has dtype {t.dtype}, expected {dtype}")
    return t, dtype


def upload(who, device, *checked):
    if torch.device(device).type != "cuda":
        raise GigaPoseHipError(f"{who} needs a GPU device (no CPU fallback)")
    return [t.to(device=device, dtype=dtype).contiguous() for t, dtype in checked]


def on_device(t, dtype, shape, who, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise GigaPoseHipError(f"{who} needs {what} on the GPU (no CPU fallback)")
    _expect(t, dtype, shape, who, what)
    return t.contiguous()


def chunked(N, limit):
    """The launches of N items at `limit` per launch (the grid's second dimension holds 65535): yields (chunk index, a, b)."""
    for c, a in enumerate(range(0, N, limit)):
        yield c, a, min(N, a + limit)


def first_bad(flags, limit):
    """Per-chunk error flags (n + 1 inside the chunk, 0 = none) -> index of a bad item, or None."""
    for c, f in enumerate(flags):
        if f:
            return c * limit + f - 1
    return None


def lib():
    global _lib, _product
    if _lib is None:
        if _product is None:
            _product = _load(LIB_PATH, "gigapose_hip.h")
        _lib = _product
    return _lib


class probe_library:
    """`with _lib.probe_library():` -- the calls of the block go to libgigapose_hip_probe.so: the same kernels built with -DGP_PROBES,
    which adds the A/B switches, traced builds, test-only epilogues and error-word readers of include/gigapose_hip_probe.h.  For tests
    that compare a kernel variant with its default bit for bit, and for tools/.  The product library carries none of those hooks;
    nothing in gigapose_amd/ or bench.py's timed region uses this."""

    def __enter__(self):
        global _lib, _probe
        lib()
        if _probe is None:
            _probe = _load(PROBE_LIB_PATH, "gigapose_hip.h", "gigapose_hip_probe.h")
        self._prev, _lib = _lib, _probe
        _reregister()
        return _probe

    def __exit__(self, *exc):
        global _lib
        _lib = self._prev
        _reregister()
        return False


def use_probe_library():
    """tools/: route every call of this process to libgigapose_hip_probe.so from here on (see probe_library)."""
    probe_library().__enter__()


STATUS_BITS = {1: "a stream-K accumulator hand-over of the split GEMM timed out (features are garbage)",
               2: "a stream-K accumulator hand-over of the f32 GEMM timed out (features are garbage)",
               4: "an activation is not finite, or (split numerics) left the range of the f16 planes (|x| >= 8190 at the default plane scale; GigaPose "
                  "re-calibrates the plane scales / falls back to Dinov2ViT.set_split_gemm('128') by itself, a bare ViT call does not)",
               8: "a detection label / template id lies outside the onboarded bank (the reference raises IndexError)",
               16: "split numerics: an IST activation left the range of the f16 planes (|x| >= 8190; on ResNet.conv_kernel = '128': |x| > 65504) "
                   "or is not finite -- use ResNet.conv_kernel = '128' for this checkpoint (GigaPose falls back by itself), beyond that numerics 'chain'"}
SPLIT_RANGE_BITS = 4 | 16
# Not a device fault, hence outside STATUS_BITS (raise_status never reports it) and outside SPLIT_RANGE_BITS: under a sharded bank the
# pose recovery's crop-transform flag (reference lib3d/torch.py:54-55) travels in the all-gathered copy of the status word, in this bit,
# so that every rank raises the reference's AssertionError in the same flush (GigaPose._run_rows, sharded_flow.py).  No kernel sets it.
CROP_TRANSFORM_BIT = 1 << 30
_status = {}          # device index -> the int32 word on that device
_registered = set()   # device indices whose word the ACTIVE library has in its per-device table


def _reregister():
    """Each library keeps its own per-device table of status words: hand the words this process already owns to the active one."""
    _registered.clear()
    for idx in list(_status):
        status_word(torch.device("cuda", idx))


def status_word(device=None):
    """The device int32 the kernels OR their guard-rail bits into (include/gigapose_hip.h: gp_set_status_buffer), one per GPU.
    The library keeps a per-device table (round 6; it held ONE process-wide pointer before): the word of a device is registered once,
    with that device current, and every launch takes the word of the device it is issued on."""
    dev = torch.device(device if device is not None else "cuda")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _status:
        _status[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    if idx not in _registered:
        with torch.cuda.device(idx):
            call("gp_set_status_buffer", _status[idx])
        _registered.add(idx)
    return _status[idx]


def take_status():
    """Read + clear the status words (a host synchronisation: call where one happens anyway); returns the OR of their bits."""
    bits = 0
    for w in _status.values():
        b = int(w.item())
        if b:
            w.zero_()
        bits |= b
    return bits


def raise_status(bits):
    bits &= ~CROP_TRANSFORM_BIT   # the caller's AssertionError, not a device fault
    if bits:
        msgs = [m for b, m in STATUS_BITS.items() if bits & b]
        raise GigaPoseHipError("device status 0x%x: %s" % (bits, "; ".join(msgs)))


def check_status():
    """Read + clear the status word and raise if a bit is set."""
    raise_status(take_status())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a contiguous CUDA tensor (None -> NULL).  call() does this by itself for a tensor; tests and old call sites spell it out."""
    return ctypes.c_void_p(0 if t is None else _address(t, "ptr"))


def ptr_table(tensors):
    """A host array of the tensors' device pointers (a `const T* const*` parameter; one NULL entry when there is no tensor), each held to ptr()'s device and
    layout check.  The caller keeps the tensors alive."""
    return (ctypes.c_void_p * max(len(tensors), 1))(*[_address(t, f"ptr_table: entry {n}") for n, t in enumerate(tensors)])


def call(name, *args):
    rc = _invoke(lib(), name, args)
    if rc != 0:
        raise GigaPoseHipError(f"{name} failed (rc={rc}): {lib().gp_last_error().decode()}")


def value(name, *args):
    """A function that returns no status (a size, a count, or nothing): its result, the arguments converted as call() converts them."""
    return _invoke(lib(), name, args)


def i(v):
    return ctypes.c_int(int(v))


def f(v):
    return ctypes.c_float(float(v))


def d(v):
    return ctypes.c_double(float(v))
