"""TBase on each crop's distinct (nn1, nn2) rows (KRRN_TBASE_DISTINCT): the four entry points against
their references, exactly, and the whole forward with the knob off against on, torch.equal on every output.

  krrn_pair_compact_i32          vs tests/pairs_ref.py (torch.unique per crop + the padding rule)
  krrn_gemm_x3_gather_live_f32   live rows vs krrn_gemm_x3_gather_f32 on the same index pairs; a dead
                                 tile keeps its sentinel, guard words around `out` stay intact
  krrn_gemm_x3_live_f32          the same against krrn_gemm_x3_f32
  krrn_tbase_tail_slot_f32       vs krrn_tbase_tail_f32 on the expanded h
"""
import pytest
import torch

from pose_estimation_amd import KRRN, _lib, make_config, ops, posenet
from pose_estimation_amd._lib import P, ptr
from pose_estimation_amd.fusion import level_sizes
from pose_estimation_amd.synthetic import init_weights, make_batch

from pairs_ref import pair_compact_ref

pytestmark = pytest.mark.gpu


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _compact(dev, ia, ib, n1, n2):
    B, npts = ia.shape
    d_ia, d_ib = ia.int().to(dev), ib.int().to(dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    pa, pb, slot = (torch.full((B, npts), -1, dtype=torch.int32, device=dev) for _ in range(3))
    _lib.call("krrn_pair_compact_i32", ptr(d_ia), ptr(d_ib), B, npts, n1, n2, ptr(cnt), ptr(pa), ptr(pb), ptr(slot),
              _stream())
    torch.cuda.synchronize()
    return cnt.cpu(), pa.cpu(), pb.cpu(), slot.cpu()


def _patterns(B, npts, n1, n2, seed):
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(npts).repeat(B, 1)
    return {"same": (torch.full((B, npts), n1 - 1), torch.full((B, npts), n2 - 2)),
            "distinct": (i % n1, i // n1),
            "random": (torch.randint(0, n1, (B, npts), generator=g), torch.randint(0, n2, (B, npts), generator=g))}


@pytest.mark.parametrize("npts", [129, 200])
@pytest.mark.parametrize("pattern", ["same", "distinct", "random"])
def test_pair_compact(dev, npts, pattern):
    B, n1, n2 = 3, 50, 13
    ia, ib = _patterns(B, npts, n1, n2, npts)[pattern]
    ref = pair_compact_ref(ia, ib, n1, n2)
    got = _compact(dev, ia, ib, n1, n2)
    if pattern == "same":
        assert ref[0].tolist() == [1] * B
    if pattern == "distinct":
        assert ref[0].tolist() == [npts] * B
    for name, r, o in zip(("cnt", "pa", "pb", "slot"), ref, got):
        assert torch.equal(r, o), name


def test_pair_compact_largest_shape(dev):
    """config 5: 4096 points, n1 = 1024, n2 = 256 (the whole 2^18-key bitmap), keys up to the last one."""
    npts, n1, n2 = 4096, 1024, 256
    g = torch.Generator().manual_seed(9)
    ia = torch.randint(0, n1, (1, npts), generator=g)
    ib = torch.randint(0, n2, (1, npts), generator=g)
    ia[0, :64], ib[0, :64] = ia[0, 64:128], ib[0, 64:128]  # some repeated pairs
    ia[0, 200], ib[0, 200] = n1 - 1, n2 - 1
    ia[0, 201], ib[0, 201] = 0, 0
    ref = pair_compact_ref(ia, ib, n1, n2)
    assert int(ref[0][0]) < npts
    got = _compact(dev, ia, ib, n1, n2)
    for name, r, o in zip(("cnt", "pa", "pb", "slot"), ref, got):
        assert torch.equal(r, o), name


B_, NPTS, K_, N_ = 3, 200, 64, 128
LIVE = [1, 200, 129]
SENT = -123.25
GUARD = 256  # floats before and after `out`


def _guarded(dev):
    buf = torch.full((2 * GUARD + B_ * NPTS * N_,), SENT, device=dev)
    return buf, buf[GUARD:GUARD + B_ * NPTS * N_].view(B_, NPTS, N_)


def _check_live(buf, out, ref):
    """Live rows equal the reference; the dead tile keeps its sentinel; the guards are intact."""
    for b, lv in enumerate(LIVE):
        assert torch.equal(out[b, :lv], ref[b, :lv]), b
    assert bool((out[0, 128:] == SENT).all())  # crop 0: rows 128..199 are a tile with no live row
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())
    assert bool(torch.isfinite(out).all())


def test_gather_live_gemm(dev):
    g = torch.Generator().manual_seed(1)
    n1, n2 = 50, 13
    T1 = torch.randn(B_, n1, K_, generator=g).to(dev)
    T2 = torch.randn(B_, n2, K_, generator=g).to(dev)
    W = (torch.randn(N_, K_, generator=g) / K_ ** 0.5).to(dev)
    bias = (0.1 * torch.randn(N_, generator=g)).to(dev)
    ia = torch.randint(0, n1, (B_, NPTS), generator=g).int().to(dev)
    ib = torch.randint(0, n2, (B_, NPTS), generator=g).int().to(dev)
    live = torch.tensor(LIVE, dtype=torch.int32, device=dev)
    w3 = ops.gemm_weights_x3(W)
    ref = torch.zeros(B_, NPTS, N_, device=dev)
    _lib.call("krrn_gemm_x3_gather_f32", ptr(ia), ptr(T1), n1 * K_, K_, ptr(ib), ptr(T2), n2 * K_, K_, NPTS, B_, K_, N_,
              ptr(w3), ptr(bias), ptr(ref), N_, 1, _stream())
    buf, out = _guarded(dev)
    _lib.call("krrn_gemm_x3_gather_live_f32", ptr(ia), ptr(T1), n1 * K_, K_, ptr(ib), ptr(T2), n2 * K_, K_, NPTS, B_,
              K_, N_, ptr(w3), ptr(bias), ptr(out), N_, 1, ptr(live), _stream())
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0
    _check_live(buf, out, ref)


def test_plain_live_gemm(dev):
    g = torch.Generator().manual_seed(2)
    A = torch.randn(B_, NPTS, K_, generator=g).to(dev)
    W = (torch.randn(N_, K_, generator=g) / K_ ** 0.5).to(dev)
    bias = (0.1 * torch.randn(N_, generator=g)).to(dev)
    live = torch.tensor(LIVE, dtype=torch.int32, device=dev)
    w3 = ops.gemm_weights_x3(W)
    ref = torch.zeros(B_, NPTS, N_, device=dev)
    _lib.call("krrn_gemm_x3_f32", ptr(A), K_, NPTS, K_, N_, ptr(w3), ptr(bias), P(0), 0, ptr(ref), N_, 1, B_,
              NPTS * K_, NPTS * N_, 0, _stream())
    buf, out = _guarded(dev)
    _lib.call("krrn_gemm_x3_live_f32", ptr(A), K_, NPTS, K_, N_, ptr(w3), ptr(bias), P(0), 0, ptr(out), N_, 1, B_,
              NPTS * K_, NPTS * N_, 0, ptr(live), _stream())
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0
    _check_live(buf, out, ref)


def test_slot_tail(dev):
    B, n, C = 3, 200, 256
    g = torch.Generator().manual_seed(3)
    cnt = [1, 200, 77]
    hd = torch.randn(B, n, C, generator=g)
    slot = torch.stack([torch.randint(0, c, (n,), generator=g) for c in cnt])
    h = torch.stack([hd[b][slot[b]] for b in range(B)]).contiguous()  # the expanded per-point rows
    w4 = torch.randn(3, C, generator=g).to(dev)
    b4 = torch.randn(3, generator=g).to(dev)
    cloud = torch.randn(B, n, 3, generator=g).to(dev)
    res = []
    for name, extra, hh in (("krrn_tbase_tail_f32", (), h), ("krrn_tbase_tail_slot_f32", (slot.int().to(dev),), hd)):
        d_h = hh.to(dev)
        pred, tres = torch.zeros(B, 3, device=dev), torch.zeros(B, n, 3, device=dev)
        _lib.call(name, ptr(d_h), *[ptr(x) for x in extra], B, n, C, ptr(w4), ptr(b4), ptr(cloud), ptr(pred), ptr(tres),
                  _stream())
        torch.cuda.synchronize()
        res.append((pred.cpu(), tres.cpu()))
    assert float(res[0][0].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_rejects(dev):
    L = _lib.lib()
    N, ok, odd, s = P(0), P(256), P(260), _stream()
    EARG, EALIGN, ESHAPE = -1, -3, -2
    pc = L.krrn_pair_compact_i32  # ia, ib, B, npts, n1, n2, cnt, pa, pb, slot, stream
    assert pc(N, ok, 1, 8, 4, 4, ok, ok, ok, ok, s) == EARG
    assert pc(ok, ok, 1, 8, 4, 4, ok, ok, ok, N, s) == EARG
    assert pc(ok, ok, 1, 8, 1024, 257, ok, ok, ok, ok, s) == ESHAPE   # past the LDS bitmap
    assert pc(ok, ok, 1, 70000, 4, 4, ok, ok, ok, ok, s) == ESHAPE
    assert pc(ok, ok, 0, 8, 4, 4, ok, ok, ok, ok, s) == ESHAPE
    gl = L.krrn_gemm_x3_live_f32
    assert gl(ok, 128, 64, 128, 128, ok, N, N, 0, ok, 128, 0, 1, 0, 0, 0, N, s) == EARG     # live NULL
    assert gl(N, 128, 64, 128, 128, ok, N, N, 0, ok, 128, 0, 1, 0, 0, 0, ok, s) == EARG
    assert gl(odd, 128, 64, 128, 128, ok, N, N, 0, ok, 128, 0, 1, 0, 0, 0, ok, s) == EALIGN
    assert gl(ok, 128, 64, 100, 128, ok, N, N, 0, ok, 128, 0, 1, 0, 0, 0, ok, s) == ESHAPE
    # ia, A, a_bs, a_st, ib, A2, a2_bs, a2_st, npts, B, K, N, w3f, bias, out, ldo, relu, live, stream
    ga = L.krrn_gemm_x3_gather_live_f32
    assert ga(ok, ok, 640, 64, ok, ok, 640, 64, 8, 1, 64, 128, ok, N, ok, 128, 0, N, s) == EARG   # live NULL
    assert ga(ok, ok, 640, 64, N, ok, 640, 64, 8, 1, 64, 128, ok, N, ok, 128, 0, ok, s) == EARG
    assert ga(ok, ok, 640, 64, ok, odd, 640, 64, 8, 1, 64, 128, ok, N, ok, 128, 0, ok, s) == EALIGN
    assert ga(ok, ok, 640, 64, ok, ok, 640, 64, 8, 1, 64, 128, ok, N, odd, 128, 0, ok, s) == EALIGN
    assert ga(ok, ok, 640, 64, ok, ok, 640, 64, 8, 1, 64, 96, ok, N, ok, 128, 0, ok, s) == ESHAPE
    ts = L.krrn_tbase_tail_slot_f32  # h, slot, B, n, C, w4, b4, cloud, pred_t, t_res, stream
    assert ts(ok, N, 1, 8, 16, ok, ok, ok, ok, N, s) == EARG
    assert ts(ok, ok, 1, 8, 16, ok, ok, ok, N, N, s) == EARG
    assert ts(odd, ok, 1, 8, 16, ok, ok, ok, ok, N, s) == EALIGN
    assert ts(ok, ok, 1, 8, 6, ok, ok, ok, ok, N, s) == EALIGN
    assert ts(ok, ok, 1, 0, 16, ok, ok, ok, ok, N, s) == ESHAPE


# ---- the whole forward: the knob off against on --------------------------------------------------------
B, S, N = 20, 64, 256


def _run(dev, sd, args, perms):
    m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    outs = []
    for _ in range(3):  # serial warm-up, capture (side streams as graph branches), replay
        outs.append({k: v.clone() for k, v in m(*args, perms=perms).items() if v is not None})
    torch.cuda.synchronize()
    plan = m.get_plan(B, S, N, True)
    bufs = {k: v.clone() for k, v in plan.fusion_bufs.items() if torch.is_tensor(v)}
    tb = {k: v.clone() for k, v in plan.tbase_bufs.items() if torch.is_tensor(v)}
    names = [op.name for op in plan.plan.ops]
    del m, plan
    torch.cuda.empty_cache()
    return outs, bufs, tb, names


def test_forward_is_bit_identical_with_both_knobs(dev, monkeypatch):
    m0 = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
    sd = init_weights(m0, 0)
    d = make_batch(B, S, N, seed=11)
    args = (d["img_croped"].to(dev), d["cloud"].to(dev), d["choose"].to(dev), d["cls_id"].to(dev))
    g = torch.Generator().manual_seed(5)
    N1, N2, _, _ = level_sizes(N, 10)
    perms = [torch.randperm(N, generator=g)[:N1] for _ in range(4)] + [torch.randperm(N1, generator=g)[:N2]]
    perms = [p.to(dev) for p in perms]
    monkeypatch.setattr(posenet, "TBASE_DISTINCT", False)
    off_outs, off_bufs, off_tb, off_names = _run(dev, sd, args, perms)
    assert "krrn_pair_compact_i32" not in off_names and "krrn_tbase_tail_f32" in off_names
    monkeypatch.setattr(posenet, "TBASE_DISTINCT", True)
    on_outs, on_bufs, on_tb, on_names = _run(dev, sd, args, perms)
    for nm in ("krrn_pair_compact_i32", "krrn_gemm_x3_gather_live_f32", "krrn_gemm_x3_live_f32",
               "krrn_tbase_tail_slot_f32"):
        assert nm in on_names, nm
    assert "pred_t" in off_outs[0]
    for r in range(3):
        for k in off_outs[0]:
            assert torch.equal(off_outs[r][k], off_outs[0][k]), (r, k)
            assert torch.equal(on_outs[r][k], off_outs[0][k]), (r, k)
    assert set(on_bufs) == set(off_bufs)
    for k in off_bufs:
        assert torch.equal(on_bufs[k], off_bufs[k]), k
    # the skip path really ran: fewer distinct pairs than points in every crop, and they are the
    # reference's (a CPU count on these inputs gives 83..94 of 256)
    cnt = on_tb["cnt"].cpu()
    print("distinct pairs per crop: min", int(cnt.min()), "mean", float(cnt.float().mean()), "max", int(cnt.max()))
    assert int(cnt.max()) < N and int(cnt.min()) >= 1
    ref = pair_compact_ref(on_bufs["nn1"], on_bufs["nn2"], N1, N2)
    for name, r in zip(("cnt", "pa", "pb", "slot"), ref):
        assert torch.equal(on_tb[name].cpu(), r), name
    # the distinct rows are the per-point path's rows: h3[b, slot[b, i]] == the per-point h3[b, i]
    slot = on_tb["slot"].long()
    for name in ("h2", "h3"):
        full = off_tb[name].view(B, N, 256)
        packed = on_tb[name].view(B, N, 256)
        assert torch.equal(torch.gather(packed, 1, slot[:, :, None].expand(B, N, 256)), full), name
