"""ctypes binding of libcheb_mi355.so (the C ABI declared in include/cheb_mi355.h).

The HIP library is the only compute path: if it is missing this module raises
ImportError -- there is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# CG_LIB_PATH: load an alternative in-tree build (kernel-variant experiments)
LIB_PATH = os.environ.get("CG_LIB_PATH") or os.path.join(_HERE, "libcheb_mi355.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cheb_mi355.h")
TESTING_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cheb_mi355_testing.h")


@functools.lru_cache(maxsize=None)
def _declarations(path: str) -> str:
    """The header's text without comments and preprocessor lines (read once)."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)


def header_enums(path: str = HEADER_PATH):
    """{NAME: value} of every enumerator in the header's ``enum { ... }`` blocks."""
    return {name: int(value) for body in re.findall(r"\benum\s*\{([^}]*)\}", _declarations(path))
            for name, value in re.findall(r"(\w+)\s*=\s*(-?\d+)", body)}


def enum_names(prefix: str, skip=()):
    """The header's enumerators under ``prefix`` by their lower-case suffix:
    enum_names("CG_PATH_") == {"auto": 0, "resident": 1, "stream": 2}."""
    return {name[len(prefix):].lower(): value for name, value in ENUMS.items()
            if name.startswith(prefix) and name not in skip}


# every CG_* constant of the public header is a module attribute (CG_OK, CG_ERR_*, ...)
ENUMS = header_enums()
globals().update(ENUMS)
PATHS = enum_names("CG_PATH_")
VARIANTS = enum_names("CG_VARIANT_")
BASIS_LAYOUTS = enum_names("CG_BASIS_")
# kernel-selection options (cg_set_option)
OPTIONS = enum_names("CG_OPT_", skip=("CG_OPT_COUNT",))


class CGError(RuntimeError):
    """A non-zero status from libcheb_mi355 (message from cg_last_error())."""

    def __init__(self, func, code, msg):
        super().__init__(f"{func} failed with status {code}: {msg}")
        self.code = code


def header_prototypes(path: str = HEADER_PATH):
    """{name: (return type, [parameter types])} of every cg_* function the header
    declares, the types as C spells them without the parameter's name
    ("const float*", "int32_t[16]")."""
    def ctype(decl):
        return re.sub(r"\s+", " ", decl).replace(" *", "*").strip()

    protos = {}
    for stmt in re.split(r"[;{}]", _declarations(path)):
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(cg_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m is None:
            continue
        ret, name, params = m.groups()
        types = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"(.*?)\w+\s*(\[\d*\])?", p.strip(), flags=re.S)
            types.append(ctype(m.group(1)) + (m.group(2) or ""))
        protos[name] = (ctype(ret), types)
    return protos


def header_symbols(path: str = HEADER_PATH):
    """Every function the public header declares (used by the ABI-export test)."""
    return sorted(header_prototypes(path))


# C type -> ctypes type.  The typed pointers are always host out-parameters, so a
# byref of the wrong type is still rejected; every other pointer (arrays included)
# is void*: the header cannot say whether it points to host or device memory
_ARGTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
             "size_t": ctypes.c_size_t, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64,
             "size_t*": ctypes.POINTER(ctypes.c_size_t), "int*": ctypes.POINTER(ctypes.c_int),
             "int64_t*": ctypes.POINTER(ctypes.c_int64),
             "cg_plan**": ctypes.POINTER(ctypes.c_void_p),
             "cg_comm**": ctypes.POINTER(ctypes.c_void_p)}
_RESTYPES = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}


def signatures(*paths: str):
    """{name: (argtypes, restype)} for every prototype of the given headers;
    ValueError for a type outside the tables above -- nothing is guessed."""
    def mapped(name, what, ctype, table):
        if ctype in table:
            return table[ctype]
        if table is _ARGTYPES and ctype.endswith(("*", "]")):
            return ctypes.c_void_p
        raise ValueError(f"{name}: no ctypes type for {what}, {ctype!r}")

    return {name: ([mapped(name, f"parameter {i}", p, _ARGTYPES) for i, p in enumerate(params)],
                   mapped(name, "the return type", ret, _RESTYPES))
            for path in paths for name, (ret, params) in header_prototypes(path).items()}


_SIGNATURES = signatures(HEADER_PATH, TESTING_HEADER_PATH)

_lib = None


def lib():
    """Load (once) and return the ctypes handle.  Raises ImportError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is not built: run `make` (or __graft_entry__.build()) -- "
            "cnn_graph_amd has no CPU/PyTorch fallback for its HIP kernels")
    h = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(h, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = h
    return h


def check(func_name: str, status: int):
    if status != CG_OK:
        msg = lib().cg_last_error()
        raise CGError(func_name, status, msg.decode() if msg else "")


def get_option(name: str) -> int:
    v = ctypes.c_int32()
    call("cg_get_option", OPTIONS[name], ctypes.byref(v))
    return v.value


def set_option(name: str, value: int) -> int:
    """Set a kernel-selection option (process-wide); returns the previous value."""
    old = get_option(name)
    call("cg_set_option", OPTIONS[name], int(value))
    return old


class options:
    """Context manager: ``with _lib.options(dw_direct=0): ...`` restores on exit."""

    def __init__(self, **kw):
        self.kw, self.saved = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.saved[k] = set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            set_option(k, v)
        return False


def call(func_name: str, *args):
    """Call a C-ABI function and raise CGError on a non-zero status."""
    status = getattr(lib(), func_name)(*args)
    check(func_name, status)
    return status
