"""The C-ABI library loads and exports every symbol include/krrn_hip.h declares, and rejects bad
arguments with the documented codes on the host side (no GPU needed: the checks run before any
HIP call)."""
import ctypes
import os
import re

import pytest

from pose_estimation_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "krrn_hip.h")


def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^int (krrn_\w+)\(", src, re.M)))


def test_header_declares_entry_points():
    names = _declared()
    assert len(names) >= 15
    assert "krrn_conv2d_f32" in names and "krrn_pnp_ransac_f32" in names


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    for name in _declared():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"


def test_ctypes_signatures_match_header_arity():
    src = open(HEADER).read()
    for name in _declared():
        m = re.search(rf"^int {name}\((.*?)\);", src, re.M | re.S)
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name]), (name, nargs, len(_lib.SIGNATURES[name]))


# the signatures of a few entry points written out by hand, independent of the parser; between them they
# use every scalar type of the ABI
_P, _I, _U, _L, _F, _D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_float,
                          ctypes.c_double)
EXPECTED = {
    "krrn_conv2d_f32": [_P] + [_I] * 10 + [_P, _P, _P, _I, _I, _P, _P, _P, _I, _P, _I, _I, _P] + [_I] * 12 + [_P, _P],
    "krrn_knn_f32": [_P, _L, _I, _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _P, _P],  # long long strides
    "krrn_pnp_ransac_f32": [_P, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _F, _D, _P, _P, _P, _P, _P, _I, _P],
    "krrn_blas_gemm_create": [_I] * 6 + [_L, _L, _I, _I, _I, _I, _L, _L, _P, _P],  # ** and * out-parameters
    "krrn_randperm_i32": [_P, _U, _I, _I, _I, _P, _P],  # unsigned int
}


def test_ctypes_signatures_match_header_types():
    assert len(EXPECTED["krrn_conv2d_f32"]) == 38
    assert {t for sig in EXPECTED.values() for t in sig} == {_P, _I, _U, _L, _F, _D}
    for name, argtypes in EXPECTED.items():
        assert _lib.SIGNATURES[name] == argtypes, name
    lib = _lib.lib()
    for name in _declared():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES[name] and fn.restype is ctypes.c_int, name


@pytest.mark.parametrize("ctype", ["short", "size_t", "unsigned", "unsigned long long", "int64_t"])
def test_parser_rejects_unknown_scalar_type(ctype):
    with pytest.raises(ValueError, match=rf"krrn_thing.*{ctype} n"):
        _lib.parse_signatures(f"int krrn_thing(const float* a, {ctype} n, void* stream);")
    ok = _lib.parse_signatures("/* int krrn_no(short n); */\nint krrn_thing(const float* a,\n    long long n); // x")
    assert ok == {"krrn_thing": [_P, _L]}


def test_register_after_load_binds_at_once():
    lib = _lib.lib()
    name = "krrn_rng_advance"
    fn, before = getattr(lib, name), _lib.SIGNATURES[name]
    try:
        fn.argtypes = None
        _lib.register(name, list(before))
        assert list(fn.argtypes) == before and fn.restype is ctypes.c_int
    finally:
        _lib.SIGNATURES[name] = before
        fn.argtypes = before


def test_host_side_errors():
    lib = _lib.lib()
    N = ctypes.c_void_p(0)
    # null pointers -> KRRN_EARG
    assert lib.krrn_knn_f32(N, 0, 3, 10, N, N, 0, 3, 10, 3, 4, 1, 0, 1, N, N) == -1
    fake = ctypes.c_void_p(16)
    # d must be 3 or 9 -> KRRN_ESHAPE
    assert lib.krrn_knn_f32(fake, 0, 3, 10, N, fake, 0, 3, 10, 4, 4, 1, 0, 1, fake, N) == -2
    # k + drop > 16 -> KRRN_ESHAPE
    assert lib.krrn_knn_f32(fake, 0, 3, 10, N, fake, 0, 3, 100, 3, 16, 1, 0, 1, fake, N) == -2
    # conv: cin not a multiple of 4 -> KRRN_EALIGN
    taps = (ctypes.c_int * 9)()
    assert lib.krrn_conv2d_f32(fake, 4, 0, 1, 8, 8, 3, 8, 8, 1, 1, taps, taps, fake, 4, 4, N, N, N, 1, N, 0, 0,
                               fake, 4, 0, 8, 8, 1, 1, 0, 0, 0, 0, 0, 1, N, N) == -3
    # pnp: P < 5 -> KRRN_ESHAPE
    assert lib.krrn_pnp_ransac_f32(fake, 16, fake, 10, fake, 4, fake, fake, fake, fake, fake, fake, 10,
                                   ctypes.c_float(1.0), ctypes.c_double(0.9999), fake, fake, fake, fake, N, 1, N) == -2
    # NCHW 1x1 split form: null weights -> KRRN_EARG; N outside (32, 80] or cin != 128 -> KRRN_ESHAPE;
    # misaligned channel offset -> KRRN_EALIGN
    nchw_x3 = lib.krrn_conv1x1_nchw_x3_f32
    assert nchw_x3(fake, 128, 0, 1, 64, 128, N, 72, 72, N, N, fake, 72, 0, N) == -1
    assert nchw_x3(fake, 128, 0, 1, 64, 128, fake, 16, 16, N, N, fake, 16, 0, N) == -2
    assert nchw_x3(fake, 256, 0, 1, 64, 256, fake, 72, 72, N, N, fake, 72, 0, N) == -2
    assert nchw_x3(fake, 136, 2, 1, 64, 128, fake, 72, 72, N, N, fake, 72, 0, N) == -3
    with pytest.raises(RuntimeError, match="KRRN_EARG"):
        _lib.check(-1, "x")
