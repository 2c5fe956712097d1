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
    # pnp: every other refusal, each before any launch. Arguments: xyz, HW, choose, N, sel, P, xmap, ymap, K4, extent,
    # lfborder, subsets, H, thr, conf, workspace, R, t, inliers, inlier_mask, B, stream
    def pnp(HW=16, N_=10, P_=5, H=10, conf=0.9999, B=1, null=None):
        a = [fake, HW, fake, N_, fake, P_, fake, fake, fake, fake, fake, fake, H, ctypes.c_float(1.0),
             ctypes.c_double(conf), fake, fake, fake, fake, N, B, N]
        if null is not None:
            assert a[null] is fake
            a[null] = N
        return lib.krrn_pnp_ransac_f32(*a)
    for bad in (dict(P_=4), dict(P_=1025), dict(H=0), dict(H=4096), dict(N_=0), dict(HW=0), dict(B=0),
                dict(conf=-0.1), dict(conf=1.1), dict(conf=float("nan"))):
        assert pnp(**bad) == -2, bad
    required = [0, 2, 4, 6, 7, 8, 9, 10, 11, 15, 16, 17, 18]  # every pointer but inlier_mask (19) and the stream
    for i in required:
        assert pnp(null=i) == -1, i
    assert pnp(null=0, P_=4) == -1  # a null pointer is reported before a bad shape
    # NCHW 1x1 split form: null weights -> KRRN_EARG; N outside (32, 80] or cin != 128 -> KRRN_ESHAPE;
    # misaligned channel offset -> KRRN_EALIGN
    nchw_x3 = lib.krrn_conv1x1_nchw_x3_f32
    assert nchw_x3(fake, 128, 0, 1, 64, 128, N, 72, 72, N, N, fake, 72, 0, N) == -1
    assert nchw_x3(fake, 128, 0, 1, 64, 128, fake, 16, 16, N, N, fake, 16, 0, N) == -2
    assert nchw_x3(fake, 256, 0, 1, 64, 256, fake, 72, 72, N, N, fake, 72, 0, N) == -2
    assert nchw_x3(fake, 136, 2, 1, 64, 128, fake, 72, 72, N, N, fake, 72, 0, N) == -3
    with pytest.raises(RuntimeError, match="KRRN_EARG"):
        _lib.check(-1, "x")


def test_point_branch_host_side_errors():
    """One call per documented rejection of the point-branch entry points: fake non-null pointers, nothing
    is launched. ok = 16-byte aligned, odd = 4 bytes off."""
    lib = _lib.lib()
    N, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68)
    EARG, ESHAPE, EALIGN = -1, -2, -3

    knn = lib.krrn_knn_f32  # q, q_bs, q_st, nq, qidx, c, c_bs, c_st, nc, d, k, drop_first, mode, B, out, stream
    assert knn(ok, 0, 3, 10, N, N, 0, 3, 10, 3, 4, 1, 0, 1, ok, N) == EARG       # c NULL
    assert knn(ok, 0, 3, 10, N, ok, 0, 3, 10, 3, 4, 1, 2, 1, ok, N) == EARG      # mode not 0 / 1
    assert knn(ok, 0, 3, 0, N, ok, 0, 3, 10, 3, 4, 1, 0, 1, ok, N) == ESHAPE     # nq = 0
    assert knn(ok, 0, 3, 10, N, ok, 0, 3, 10, 3, 4, 1, 0, -1, ok, N) == ESHAPE   # B < 0
    assert knn(ok, 0, 3, 10, N, ok, 0, 3, 4, 3, 4, 1, 0, 1, ok, N) == ESHAPE     # k + drop = 5 > nc = 4
    assert knn(ok, 0, 3, 10, N, ok, 0, 3, 4, 3, 5, 0, 0, 1, ok, N) == ESHAPE     # k = 5 > nc = 4

    # idx, n, k, v, v_bs, v_st, d, dn, S, C, Y, bn_scale, bn_bias, relu, out, o_bs, o_st, B, stream
    gcn = lib.krrn_gcn_conv_f32
    assert gcn(ok, 8, 4, ok, 24, 3, 3, N, 7, 128, N, N, N, 0, ok, 1024, 128, 1, N) == EARG        # dn NULL
    assert gcn(ok, 8, 4, ok, 24, 3, 3, ok, 7, 128, N, ok, N, 0, ok, 1024, 128, 1, N) == EARG      # scale without bias
    assert gcn(ok, 8, 4, ok, 24, 3, 4, ok, 7, 128, N, N, N, 0, ok, 1024, 128, 1, N) == ESHAPE     # d = 4
    assert gcn(ok, 0, 4, ok, 24, 3, 3, ok, 7, 128, N, N, N, 0, ok, 1024, 128, 1, N) == ESHAPE     # n = 0
    assert gcn(ok, 8, 17, ok, 24, 3, 3, ok, 7, 128, N, N, N, 0, ok, 1024, 128, 1, N) == ESHAPE    # k > 16
    assert gcn(ok, 8, 4, ok, 24, 3, 3, ok, 7, 126, N, N, N, 0, ok, 1024, 128, 1, N) == EALIGN     # C % 4
    assert gcn(ok, 8, 4, ok, 24, 3, 3, ok, 7, 128, N, N, N, 0, ok, 1024, 130, 1, N) == EALIGN     # o_st % 4
    assert gcn(ok, 8, 4, ok, 24, 3, 3, ok, 7, 128, N, N, N, 0, odd, 1024, 128, 1, N) == EALIGN    # out misaligned
    assert gcn(ok, 8, 4, ok, 24, 3, 3, ok, 7, 128, odd, N, N, 0, ok, 1024, 128, 1, N) == EALIGN   # Y misaligned

    pool = lib.krrn_pool_max_f32  # nbr, nq, kk, F, f_bs, f_st, C, out, o_bs, o_st, B, stream
    assert pool(ok, 8, 4, N, 1024, 128, 128, ok, 1024, 128, 1, N) == EARG        # F NULL
    assert pool(ok, 8, 0, ok, 1024, 128, 128, ok, 1024, 128, 1, N) == ESHAPE     # kk = 0
    assert pool(ok, -1, 4, ok, 1024, 128, 128, ok, 1024, 128, 1, N) == ESHAPE    # nq < 0
    assert pool(ok, 8, 4, ok, 1024, 128, 6, ok, 1024, 128, 1, N) == EALIGN       # C % 4
    assert pool(ok, 8, 4, ok, 1024, 130, 128, ok, 1024, 128, 1, N) == EALIGN     # f_st % 4
    assert pool(ok, 8, 4, odd, 1024, 128, 128, ok, 1024, 128, 1, N) == EALIGN    # F misaligned

    # in, B, Hi, Wi, in_cs, in_co, C, out, Ho, Wo, out_cs, out_co, add, add_cs, add_co, align_corners, relu, stream
    rs = lib.krrn_resize_bilinear_f32
    assert rs(N, 1, 4, 4, 8, 0, 8, ok, 8, 8, 8, 0, N, 0, 0, 0, 0, N) == EARG         # in NULL
    assert rs(ok, 1, 4, 4, 8, 0, 8, ok, 0, 8, 8, 0, N, 0, 0, 0, 0, N) == ESHAPE      # Ho = 0
    assert rs(ok, 1, 4, 4, 8, 0, 6, ok, 8, 8, 8, 0, N, 0, 0, 0, 0, N) == EALIGN      # C % 4
    assert rs(ok, 1, 4, 4, 8, 2, 4, ok, 8, 8, 8, 0, N, 0, 0, 0, 0, N) == EALIGN      # in_co % 4
    assert rs(ok, 1, 4, 4, 8, 0, 8, odd, 8, 8, 8, 0, N, 0, 0, 0, 0, N) == EALIGN     # out misaligned
    assert rs(ok, 1, 4, 4, 8, 0, 8, ok, 8, 8, 8, 0, odd, 8, 0, 0, 0, N) == EALIGN    # add misaligned

    ar = lib.krrn_add_relu_f32  # a, a_cs, a_co, b, b_cs, b_co, out, o_cs, o_co, npix, C, relu, stream
    assert ar(N, 8, 0, N, 0, 0, ok, 8, 0, 4, 8, 0, N) == EARG          # a NULL
    assert ar(ok, 8, 0, N, 0, 0, N, 8, 0, 4, 8, 0, N) == EARG          # out NULL
    assert ar(ok, 8, 0, N, 0, 0, ok, 8, 0, 0, 8, 0, N) == ESHAPE       # npix = 0
    assert ar(ok, 8, 0, N, 0, 0, ok, 8, 0, 4, 6, 0, N) == EALIGN       # C % 4
    assert ar(ok, 8, 0, ok, 8, 2, ok, 8, 0, 4, 4, 0, N) == EALIGN      # b_co % 4
    assert ar(odd, 8, 0, N, 0, 0, ok, 8, 0, 4, 8, 0, N) == EALIGN      # a misaligned (float4 loads)
    assert ar(ok, 8, 0, odd, 8, 0, ok, 8, 0, 4, 8, 0, N) == EALIGN     # b misaligned
    assert ar(ok, 8, 0, N, 0, 0, odd, 8, 0, 4, 8, 0, N) == EALIGN      # out misaligned (float4 stores)

    to_nhwc = lib.krrn_nchw_to_nhwc_f32  # in, B, C, H, W, out, o_cs, o_co, stream
    assert to_nhwc(ok, 1, 3, 4, 4, N, 4, 0, N) == EARG             # out NULL
    assert to_nhwc(ok, 1, 3, 0, 4, ok, 4, 0, N) == ESHAPE          # H = 0
    assert to_nhwc(ok, 1, 3, 4, 4, ok, 4, 2, N) == ESHAPE          # o_co + C = 5 > o_cs = 4

    # fx, Cx, xyz_off, fn, Cn, cls, xyz_out, nml_out, B, H, W, stream
    hs = lib.krrn_heads_select_f32
    assert hs(ok, 24, 7, ok, 15, N, ok, ok, 1, 4, 4, N) == EARG        # cls NULL
    assert hs(ok, 24, 7, ok, 15, ok, ok, ok, 0, 4, 4, N) == ESHAPE     # B = 0
    assert hs(ok, 9, 7, ok, 15, ok, ok, ok, 1, 4, 4, N) == ESHAPE      # Cx = 9 < xyz_off + 3 = 10
    assert hs(ok, 24, 7, ok, 2, ok, ok, ok, 1, 4, 4, N) == ESHAPE      # Cn < 3

    pg = lib.krrn_points_gather_f32  # cloud, xyz, nml, choose, B, N, H, W, p9, stream
    assert pg(ok, ok, ok, N, 1, 8, 4, 4, ok, N) == EARG            # choose NULL
    assert pg(ok, ok, ok, ok, 1, 8, 4, 4, N, N) == EARG            # p9 NULL
    assert pg(ok, ok, ok, ok, 1, 0, 4, 4, ok, N) == ESHAPE         # N = 0

    # idx, idx64, idx_bs, nrows, src, src_bs, src_st, dst, dst_bs, dst_st, width, B, stream
    gr = lib.krrn_gather_rows_f32
    assert gr(N, 0, 0, 8, ok, 64, 8, ok, 64, 8, 8, 1, N) == EARG       # idx NULL
    assert gr(ok, 0, 0, 8, N, 64, 8, ok, 64, 8, 8, 1, N) == EARG       # src NULL
    assert gr(ok, 0, 0, 0, ok, 64, 8, ok, 64, 8, 8, 1, N) == ESHAPE    # nrows = 0
    assert gr(ok, 1, 0, 8, ok, 64, 8, ok, 64, 8, -4, 1, N) == ESHAPE   # width < 0

    # ia, A, a_bs, a_st, ib, B_, b_bs, b_st, n, C, scale, bias, bias2, relu, out, o_bs, o_st, B, stream
    g2 = lib.krrn_gather2_add_f32
    assert g2(ok, ok, 64, 8, N, ok, 64, 8, 4, 8, ok, ok, N, 0, ok, 64, 8, 1, N) == EARG        # ib NULL
    assert g2(ok, ok, 64, 8, ok, ok, 64, 8, 4, 8, ok, N, N, 0, ok, 64, 8, 1, N) == EARG        # bias NULL
    assert g2(ok, ok, 64, 8, ok, ok, 64, 8, 0, 8, ok, ok, N, 0, ok, 64, 8, 1, N) == ESHAPE     # n = 0
    assert g2(ok, ok, 64, 8, ok, ok, 64, 8, 4, 6, ok, ok, N, 0, ok, 64, 8, 1, N) == EALIGN     # C % 4
    assert g2(ok, ok, 64, 8, ok, ok, 66, 8, 4, 8, ok, ok, N, 0, ok, 64, 8, 1, N) == EALIGN     # b_bs % 4
    assert g2(ok, ok, 64, 8, ok, ok, 64, 8, 4, 8, ok, ok, N, 0, ok, 64, 10, 1, N) == EALIGN    # o_st % 4
    assert g2(ok, odd, 64, 8, ok, ok, 64, 8, 4, 8, ok, ok, N, 0, ok, 64, 8, 1, N) == EALIGN    # A misaligned
    assert g2(ok, ok, 64, 8, ok, ok, 64, 8, 4, 8, ok, ok, odd, 0, ok, 64, 8, 1, N) == EALIGN   # bias2 misaligned

    tt = lib.krrn_tbase_tail_f32  # h, B, n, C, w4, b4, cloud, pred_t, t_res, stream
    assert tt(ok, 1, 8, 16, ok, ok, N, ok, N, N) == EARG           # cloud NULL
    assert tt(ok, 1, 8, 16, ok, ok, ok, N, N, N) == EARG           # pred_t NULL (t_res is optional)
    assert tt(ok, 1, 0, 16, ok, ok, ok, ok, N, N) == ESHAPE        # n = 0
    assert tt(ok, 1, 8, 6, ok, ok, ok, ok, N, N) == EALIGN         # C % 4
    assert tt(odd, 1, 8, 16, ok, ok, ok, ok, N, N) == EALIGN       # h misaligned
    assert tt(ok, 1, 8, 16, odd, ok, ok, ok, N, N) == EALIGN       # w4 misaligned
