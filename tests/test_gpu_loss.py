"""csrc/loss.hip against the f64 restatements of tests/loss_ref.py at the block, tile and branch
edges (GPU). The inputs are loss_ref's builders, whose worth tests/test_loss_ref_host.py shows on the
CPU: a dropped boundary pixel or tile-edge candidate, a swapped matching direction or another crop's
records would miss these tolerances by a factor of 100 or more.

Map terms: 2e-6 relative per value, the project's tolerance for them (the f32 oracle stays within
1.1e-7 of f64 on random maps of these shapes; the kernel sums in f64), counts exact.
Point terms: loss_ref.point_tol per value: the largest of 4 x the f32 torch restatement's own error
on the same inputs, 8 * 2^-24 * max |coordinate| and 2e-6 relative. Measured on the CPU, the f32
restatement's error against f64 over the cases here (max |coordinate| 6.0 to 8.0 m: the isolated
tile-edge points of loss_ref.edge_points; the second term is 2.9e-6 to 3.8e-6): at B = 3 PoseLoss
1.7e-7 and ADD(-S) 3.6e-7 for P = 1 (a single pair 1 cm apart at 6 m), PoseLoss <= 1.7e-9 and ADD(-S)
<= 3.5e-9 for P in {255 ... 4097}; PoseLoss 6.4e-13 and ADD(-S) <= 2.4e-8 at B = 300, P = 37; 1.2e-9 and
1.6e-8 in the sym=[] case. 4 x the f32 restatement's error never exceeds the second term, so the
coordinate term is the bound everywhere. On the edge maps the f32 oracle is within 1.4e-8 (xyz),
4.5e-7 (normal), 9.4e-8 (region) and 1.4e-7 (mask) of f64, relative."""
import ctypes

import pytest
import torch

import loss_ref as lr

MAP_SHAPES = [(3, 64, 64, 7, 4), (3, 17, 241, 7, 4), (2, 64, 129, 65, 22), (130, 17, 241, 2, 2), (2, 1, 5, 3, 2)]
POINT_P = [1, 255, 256, 257, 2048, 2049, 4096, 4097]
SYM3 = [False, True, True]

pytestmark = pytest.mark.gpu


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _check_terms(tag, got, val, cnt):
    """got f64 [..., 8] against the reference values and counts."""
    got = got.cpu()
    assert torch.equal(got[..., 4:], cnt.double()), (tag, got[..., 4:], cnt)
    empty = cnt == 0
    assert (got[..., :4][empty] == 0.0).all(), (tag, got[..., :4][empty])  # 0.0, not NaN
    rel = ((got[..., :4] - val).abs() / val.abs().clamp_min(1e-300))[~empty]
    print(f"{tag}: max relative error {float(rel.max()):.2e} (bound {lr.MAP_RTOL:.0e})")
    assert (rel <= lr.MAP_RTOL).all(), (tag, rel)


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_losses_edge_shapes(dev, shape):
    """One block exactly, a second block of one pixel, three blocks at the model's widths, more than
    256 partial records, a tile far smaller than a block: pooled and per-crop terms."""
    from pose_estimation_amd.loss import map_losses
    pred, gt = lr.edge_maps(*shape, seed=11)
    s, n = lr.map_terms(pred, gt)
    pd, gd = _to(pred, dev), _to(gt, dev)
    _check_terms(f"pooled {shape}", map_losses(pd, gd), *lr.pooled(s, n))
    got = map_losses(pd, gd, per_crop=True)
    assert got.shape == (shape[0], 8)
    _check_terms(f"per crop {shape}", got, *lr.per_crop(s, n))


@pytest.mark.parametrize("empty_mask", [False, True])
def test_map_losses_branches(dev, empty_mask):
    """loss_ref.branch_maps: +-90 logits, underflowing and unit probabilities, a zero predicted
    normal, a 1e-9 and a -0.0 target, labels -1 and C, an empty term (0.0 with count 0, where the
    torch restatement gives NaN)."""
    from pose_estimation_amd.loss import map_losses
    pred, gt = lr.branch_maps(empty_mask)
    s, n = lr.map_terms(pred, gt)
    pd, gd = _to(pred, dev), _to(gt, dev)
    _check_terms(f"branches pooled (empty_mask={empty_mask})", map_losses(pd, gd), *lr.pooled(s, n))
    _check_terms(f"branches per crop (empty_mask={empty_mask})", map_losses(pd, gd, per_crop=True), *lr.per_crop(s, n))


def test_map_losses_null_terms_raw_abi(dev):
    """NULL xyz and mask maps: out[0], out[3] and their counts are 0 (over a NaN-filled out), the
    other two terms are what they are with all four maps given."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import ptr, stream_ptr
    B, H, W, R, M = 2, 64, 129, 65, 22
    pred, gt = lr.edge_maps(B, H, W, R, M, seed=11)
    val, cnt = lr.pooled(*lr.map_terms(pred, gt))
    val, cnt = val.clone(), cnt.clone()
    val[0] = val[3] = 0.0
    cnt[0] = cnt[3] = 0
    HW = H * W
    nws = ctypes.c_longlong(0)
    _lib.call("krrn_map_losses_ws", B, HW, ctypes.byref(nws))
    ws = torch.full((int(nws.value),), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((8,), float("nan"), dtype=torch.float64, device=dev)
    nml, nml_gt = pred["normal"].to(dev).contiguous(), gt["normal"].to(dev).contiguous()
    reg, reg_gt = pred["region"].to(dev).contiguous(), gt["region"].to(dev).long().reshape(B, HW).contiguous()
    _lib.call("krrn_map_losses_f32", None, None, ptr(nml), ptr(nml_gt), ptr(reg), R, ptr(reg_gt), None, M, None, B, HW,
              ptr(ws), ptr(out), stream_ptr(dev))
    _check_terms("NULL xyz and mask", out, val, cnt)


def test_map_losses_bit_reproducible(dev):
    from pose_estimation_amd.loss import map_losses
    pred, gt = lr.edge_maps(130, 17, 241, 2, 2, seed=11)
    pd, gd = _to(pred, dev), _to(gt, dev)
    a, ac = map_losses(pd, gd).cpu(), map_losses(pd, gd, per_crop=True).cpu()
    b, bc = map_losses(pd, gd).cpu(), map_losses(pd, gd, per_crop=True).cpu()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(ac.view(torch.int64), bc.view(torch.int64))


def _check_points(tag, dev, case, sym_mask, cls, sym):
    from pose_estimation_amd.loss import pose_loss
    from pose_estimation_amd.metric import add_metric
    R, t, mp, tg = case
    ref = lr.points_ref(R, t, mp, tg, sym_mask)
    r32 = lr.points_ref(R, t, mp, tg, sym_mask, dtype=torch.float32)
    mc = lr.max_coord(R, t, mp, tg)
    cls = torch.tensor(cls).view(-1, 1)
    got = float(pose_loss(R.to(dev), t.to(dev), tg.to(dev), mp.to(dev), cls.to(dev), sym))
    want, w32 = ref["pose"].mean(), r32["pose"].mean()
    tol = float(lr.point_tol(want, w32, mc))
    print(f"{tag} PoseLoss: error {abs(got - float(want)):.2e}, f32 restatement {abs(float(w32 - want)):.2e}, "
          f"bound {tol:.2e} (max |coordinate| {mc:.2f})")
    assert abs(got - float(want)) <= tol, (tag, got, float(want), tol)
    got = add_metric(R.to(dev), t.to(dev), mp.to(dev), tg.to(dev), cls.to(dev), sym).cpu()
    want, w32 = lr.add_metric_ref(ref, sym_mask), lr.add_metric_ref(r32, sym_mask)
    tol = lr.point_tol(want, w32, mc)
    err = (got - want).abs()
    print(f"{tag} ADD(-S): max error {float(err.max()):.2e}, f32 restatement {float((w32 - want).abs().max()):.2e}, "
          f"bound {float(tol.min()):.2e}")
    assert (err <= tol).all(), (tag, err, tol)


@pytest.mark.parametrize("P", POINT_P)
def test_pose_loss_and_add_block_and_tile_edges(dev, P):
    """One non-symmetric and two symmetric crops at the sizes around a 256-query block and a
    2048-candidate tile, on loss_ref.edge_points."""
    _check_points(f"P={P}", dev, lr.edge_points(3, P, SYM3, seed=100 + P), SYM3, [3, 1, 2], [1, 2])


def test_pose_loss_and_add_many_crops(dev):
    """B = 300 > 256: the strided loop of pose_loss_final_kernel, the second block of
    add_metric_final_kernel; classes mixed."""
    g = torch.Generator().manual_seed(9)
    cls = torch.randint(0, 6, (300,), generator=g).tolist()
    sym = [1, 4]
    sym_mask = [c in sym for c in cls]
    assert 50 < sum(sym_mask) < 250 and not sym_mask[cls.index(0)]
    _check_points("B=300", dev, lr.edge_points(300, 37, sym_mask, seed=37), sym_mask, cls, sym)


def test_empty_sym_list_keeps_class_zero_plain(dev):
    """sym=[] reaches the kernels as the placeholder [0] with nsym = 0: class 0 is then not
    symmetric. The two crops' targets are a different point set, so ADD and ADD-S differ by more than
    1e-2 (tests/test_loss_ref_host.py)."""
    _check_points("sym=[]", dev, lr.edge_points(2, 300, [True, True], seed=5), [False, False], [0, 0], [])
