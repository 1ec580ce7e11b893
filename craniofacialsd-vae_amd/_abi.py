"""ctypes binding of ``libcfsd.so`` (the C ABI declared in ``include/cfsd.h``).

The library is built in-tree (``csrc/Makefile``, ``__graft_entry__.build()``)
and this module refuses to run without it: there is no CPU or PyTorch
fallback for any kernel.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFSD_LIB_PATH") or os.path.join(_HERE, "libcfsd.so")

HEADER_PATH = os.environ.get("CFSD_HEADER_PATH") or os.path.join(os.path.dirname(_HERE), "include", "cfsd.h")

_lib = None


class CfsdError(RuntimeError):
    pass


# ---------------------------------------------------------------- the ABI, read from cfsd.h
# The header is the one statement of the ABI: the prototypes, cfsd_dw_slabs and the integer
# CFSD_* constants below are parsed from its text.  The parser knows the few C types the
# header uses and refuses (CfsdError naming the declaration) whatever it does not know.
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
            "unsigned long long": ctypes.c_ulonglong}
_RETURNS = {**_SCALARS, "const char *": ctypes.c_char_p}
_PROTO = re.compile(r"([\w\s*]+?)\b(cfsd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(CFSD_\w+)(\(?)(.*)$", re.M)


def _ctype(decl, where):
    """ctypes type of one parameter or field (``type [name]``): any pointer is a c_void_p."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words and "[" not in decl:
        return ctypes.c_void_p
    for ty in (" ".join(words), " ".join(words[:-1])):
        if ty in _SCALARS and "[" not in decl:
            return _SCALARS[ty]
    raise CfsdError(f"cfsd.h: {where}: unsupported type in '{' '.join(decl.split())}'")


def _fields(body, where):
    """ctypes ``_fields_`` of a struct body; one declaration may name several scalar fields."""
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (d.strip() for d in decl.split(","))
        names = [first.replace("*", " ").split()[-1], *more]
        if not all(re.fullmatch(r"[A-Za-z_]\w*", n) for n in names) or (more and "*" in decl):
            raise CfsdError(f"cfsd.h: {where}: cannot read the field declaration '{decl}'")
        out += [(n, _ctype(first, where)) for n in names]
    return out


def parse_header(text):
    """(signatures {name: (restype, [argtypes])}, structs {name: _fields_}, constants {CFSD_X: int})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace("\\\n", " ")
    constants = {}
    for name, call, body in _DEFINE.findall(text):
        if call or not body.strip():  # function-like macro / include guard
            continue
        m = re.fullmatch(r"\(\s*(-?\w+)\s*\)|(-?\w+)", body.strip())
        try:
            constants[name] = int(m.group(1) or m.group(2), 0)
        except (AttributeError, ValueError):
            raise CfsdError(f"cfsd.h: #define {name} {body.strip()}: not an integer constant") from None
    code = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {name: _fields(body, name) for body, name in _STRUCT.findall(code)}
    signatures = {}
    for ret, name, params in _PROTO.findall(_STRUCT.sub("", code)):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise CfsdError(f"cfsd.h: {name}: unsupported return type '{ret}'")
        params = [p.strip() for p in params.split(",")]
        signatures[name] = (_RETURNS[ret], [] if params == ["void"] else [_ctype(p, name) for p in params])
    # a declaration the prototype pattern cannot consume must not drop out silently
    seen = re.findall(r"(cfsd_[a-z0-9_]+)\s*\(", code)
    if len(seen) != len(signatures):
        lost = sorted(set(seen) - set(signatures)) or sorted(n for n in set(seen) if seen.count(n) > 1)
        raise CfsdError(f"cfsd.h: {len(seen)} cfsd_*( declarations but {len(signatures)} prototypes read: {lost}")
    return signatures, structs, constants


try:
    with open(HEADER_PATH) as _f:
        SIGNATURES, _structs, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise CfsdError(f"cannot read the C ABI from {HEADER_PATH} (set CFSD_HEADER_PATH): {e}") from None
if "cfsd_dw_slabs" not in _structs:
    raise CfsdError(f"{HEADER_PATH}: no 'typedef struct {{ ... }} cfsd_dw_slabs;' found")
DwSlabs = type("DwSlabs", (ctypes.Structure,), {
    "__doc__": "``cfsd_dw_slabs`` (include/cfsd.h): one deferred weight-gradient slab set.",
    "_fields_": _structs["cfsd_dw_slabs"]})


def load(path=LIB_PATH):
    """Load libcfsd.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise CfsdError(
            f"{path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C csrc)")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def lib():
    return _lib if _lib is not None else load()


def check(rc, what=""):
    if rc != 0:
        msg = lib().cfsd_last_error_string().decode(errors="replace")
        raise CfsdError(f"{what or 'cfsd'} failed (rc={rc}): {msg}")


def ptr(t):
    """Device pointer of a CUDA(HIP) tensor, or None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise CfsdError("cfsd kernels take device tensors only")
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


_trace = None  # list of (name, args, start_event, end_event) while tracing


class trace_launches:
    """Context manager recording every libcfsd launch with a HIP event pair on
    the launch stream (per-kernel device time of an eager step; measurement
    only -- the product path never enables it)."""

    def __enter__(self):
        global _trace
        self.records = []
        _trace = self.records
        return self.records

    def __exit__(self, *exc):
        global _trace
        _trace = None
        return False


def call(name, *args):
    if _trace is None:
        check(getattr(lib(), name)(*args), name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(getattr(lib(), name)(*args), name)
    e1.record()
    _trace.append((name, args, e0, e1))
