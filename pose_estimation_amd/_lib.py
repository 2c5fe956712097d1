"""Loader for the in-tree C-ABI library ``libkrrn_hip.so`` (include/krrn_hip.h).

The library is the product path: there is no CPU or PyTorch fallback. If it is
missing, ``lib()`` raises immediately so that a mis-built GPU box fails loudly
instead of silently computing something else.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

import torch  # loads the HIP runtime libamdhip64.so.7 before our library

from . import knobs

P = ctypes.c_void_p


def ptr(t) -> P:
    return P(t.data_ptr()) if t is not None else P(0)


def stream_ptr(device=None) -> P:
    """The current torch stream of `device` (None: the current device), as the `hipStream_t` argument."""
    return P(torch.cuda.current_stream(device).cuda_stream)


_HERE = os.path.dirname(os.path.abspath(__file__))
# KRRN_HIP_LIB: an alternative build of the same library (kernel-variant experiments)
LIB_PATH = knobs.text("KRRN_HIP_LIB") or os.path.join(_HERE, "libkrrn_hip.so")

_lock = threading.Lock()
_lib = None

_ERRORS = {-1: "KRRN_EARG (null pointer / bad argument)",
           -2: "KRRN_ESHAPE (dimension outside the supported range)",
           -3: "KRRN_EALIGN (16-byte alignment / channel stride violation)",
           -4: "KRRN_EUNSUPPORTED (a form the kernel does not offer)"}

# include/krrn_hip.h is the ABI, and the ctypes signatures are read from it: every declaration there is
# `int krrn_name(type name, ...);` with a pointer or one of these scalar types per parameter
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "krrn_hip.h")
_SCALARS = {"int": ctypes.c_int, "unsigned int": ctypes.c_uint, "long long": ctypes.c_longlong,
            "float": ctypes.c_float, "double": ctypes.c_double}


def parse_signatures(src: str) -> dict:
    """C declarations `int krrn_*(...);` -> {name: argtypes}. Every entry point returns int. Raises on a
    parameter that is neither a pointer nor one of _SCALARS (not a C parser: the header is that regular)."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    sigs = {}
    for name, params in re.findall(r"\bint\s+(krrn_\w+)\s*\(([^()]*)\)\s*;", src):
        argtypes = []
        for param in params.split(","):
            words = param.split()
            if "*" in param:
                argtypes.append(ctypes.c_void_p)
            elif " ".join(words[:-1]) in _SCALARS:  # the last word is the parameter's name
                argtypes.append(_SCALARS[" ".join(words[:-1])])
            else:
                raise ValueError(f"{name}: no ctypes type for parameter '{' '.join(words)}'")
        sigs[name] = argtypes
    return sigs


with open(_HEADER) as _f:
    SIGNATURES = parse_signatures(_f.read())  # name -> argtypes


def _bind(handle, name, argtypes):
    fn = getattr(handle, name)
    fn.argtypes = argtypes
    fn.restype = ctypes.c_int


def register(name, argtypes):
    """Signature of a symbol the public header does not declare (a diagnostics build's krrn_diag.h)."""
    with _lock:
        SIGNATURES[name] = argtypes
        if _lib is not None:
            _bind(_lib, name, argtypes)


def lib():
    """Return the loaded library (raises RuntimeError when it is not built)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(the KRRN HIP path has no fallback)")
            handle = ctypes.CDLL(LIB_PATH)
            for name, argtypes in SIGNATURES.items():
                _bind(handle, name, argtypes)
            _lib = handle
    return _lib


def check(status: int, name: str):
    if status != 0:
        msg = _ERRORS.get(status, f"hipError_t {status}")
        raise RuntimeError(f"{name} failed: {msg}")


def call(name: str, *args):
    fn = getattr(lib(), name)
    check(fn(*args), name)
