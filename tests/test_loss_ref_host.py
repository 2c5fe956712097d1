"""tests/loss_ref.py pinned on the CPU: the f64 restatements against the project's f32 oracles on
ordinary inputs, and the edge inputs against the conditions that make them worth running, stated as
mutations of the reference's own input. A kernel that dropped a block's first or last pixel, a tile's
first or last candidate, matched in the wrong direction or read another crop's records would move
the result by at least 100 x the tolerance tests/test_gpu_loss.py allows. No GPU, no kernel: these
are properties of the inputs."""
import numpy as np
import pytest
import torch

import loss_ref as lr
from oracle import loss_oracle as lo
from test_loss import _maps, _pose_inputs
from test_metric import _ref_adds

MAP_SHAPES = [(3, 64, 64, 7, 4), (3, 17, 241, 7, 4), (2, 64, 129, 65, 22), (130, 17, 241, 2, 2), (2, 1, 5, 3, 2)]
POINT_P = [1, 255, 256, 257, 2048, 2049, 4096, 4097]
SYM3 = [False, True, True]
MARGIN = 100


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("shape", [(2, 23, 17, 7, 4), (3, 17, 241, 7, 4)])
def test_map_terms_agree_with_oracle(shape):
    pred, gt = _maps(*shape, seed=1)
    ref = lo.krrn_loss(pred, gt, [], opt_pose=False)
    s, n = lr.map_terms(pred, gt)
    val, cnt = lr.pooled(s, n)
    for i, k in enumerate(("loss_xyz", "loss_normal", "loss_region", "loss_mask")):
        assert _rel(ref[k], val[i]) < lr.MAP_RTOL, (k, float(ref[k]), float(val[i]))
    assert int(cnt[2]) == int((gt["region"] != 0).sum())
    # per crop: the oracle on crop b alone
    pv, _ = lr.per_crop(s, n)
    for b in range(shape[0]):
        ref = lo.krrn_loss({k: v[b:b + 1] for k, v in pred.items()}, {k: v[b:b + 1] for k, v in gt.items()}, [],
                           opt_pose=False)
        for i, k in enumerate(("loss_xyz", "loss_normal", "loss_region", "loss_mask")):
            assert _rel(ref[k], pv[b, i]) < lr.MAP_RTOL


def test_block_records_sum_to_the_crop_terms():
    pred, gt = lr.edge_maps(2, 64, 129, 65, 22, seed=3)
    s, n = lr.map_terms(pred, gt)
    bs, bn = lr.block_records(pred, gt)
    assert bs.shape == (2, 3, 4)
    assert torch.allclose(bs.sum(1), s, rtol=1e-13, atol=0) and torch.equal(bn.sum(1), n)


def test_point_terms_agree_with_oracles():
    B, P = 3, 300
    Rm, pt, tgt, mp, cls = _pose_inputs(B, P, 2, [1, 3, 2])
    sym_mask = [True, False, True]
    ref = lr.points_ref(Rm, pt, mp, tgt, sym_mask)
    want = lo.pose_loss(Rm, pt.unsqueeze(1), tgt, mp, cls.view(-1), [1, 2])
    assert _rel(want, ref["pose"].mean()) < 1e-5
    got = lr.add_metric_ref(ref, sym_mask)
    for b in range(B):
        pred = mp[b] @ Rm[b].t() + pt[b]
        assert _rel(_ref_adds(pred, tgt[b], sym_mask[b]), got[b]) < lr.MAP_RTOL
    # the f32 form of the same function is those oracles' arithmetic
    r32 = lr.points_ref(Rm, pt, mp, tgt, sym_mask, dtype=torch.float32)
    assert _rel(r32["pose"].mean(), ref["pose"].mean()) < 1e-5


@pytest.fixture(scope="module", params=MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def edge_case(request):
    shape = request.param
    pred, gt = lr.edge_maps(*shape, seed=11)
    return shape, pred, gt, lr.map_pixels(pred, gt), lr.map_terms(pred, gt)


def _live_boundary(shape):
    B, H, W = shape[:3]
    eb = lr.empty_block(B, H * W)
    for b in range(B):
        for p in lr.boundary_pixels(H * W):
            if eb is None or not (b == eb[0] and p // lr.BLOCK == eb[1]):
                yield b, p


def test_edge_maps_structure(edge_case):
    shape, pred, gt, (loss, valid), (s, n) = edge_case
    B, H, W = shape[:3]
    HW = H * W
    frac = valid[0, 0].double().mean()  # crop 0 has no emptied block
    assert 0.5 < frac < 0.7 or HW < 100
    eb = lr.empty_block(B, HW)
    if eb is not None:  # a whole block without a valid pixel, for every term
        assert not valid[:, eb[0], eb[1] * lr.BLOCK:(eb[1] + 1) * lr.BLOCK].any()
    assert int(n[B - 1, 3]) == 0 and float(lr.per_crop(s, n)[0][B - 1, 3]) == 0.0  # a term without a valid pixel
    assert (n[:, :3] > 0).all()
    bp = torch.tensor(lr.boundary_pixels(HW))
    for b, p in _live_boundary(shape):
        for k in range(4):
            if k == 3 and b == B - 1:
                continue
            assert valid[k, b, p]
            inner = valid[k, b].clone()
            inner[bp] = False
            if int(inner.sum()) >= 20:  # "typical": the crop's valid pixels that are no boundary pixel
                assert loss[k, b, p] >= 20 * loss[k, b][inner].mean(), (k, b, p)


def test_edge_maps_boundary_pixel_mutations(edge_case):
    """Invalidating any one boundary pixel moves each term of its crop (the per-crop output), and for
    the small batches each pooled term, by >= 100 x 2e-6. (Pooled over 130 crops one pixel among
    320 000 cannot reach that for the bounded terms: 1 - cos <= 2 and CE <= 13.8 hold it under 70 x the
    typical value; there the per-crop output carries the check.)"""
    shape, pred, gt, _, (s, n) = edge_case
    B = shape[0]
    crop0, pool0 = lr.per_crop(s, n)[0], lr.pooled(s, n)[0]
    todo = list(_live_boundary(shape))
    if B > 3:
        todo = [(b, p) for b, p in todo if b in (0, 1, 127, 128, B - 1)]
    for b, p in todo:
        s2, n2 = lr.map_terms(pred, lr.invalidate(gt, b, p))
        crop1, pool1 = lr.per_crop(s2, n2)[0], lr.pooled(s2, n2)[0]
        for k in range(4):
            if k == 3 and b == B - 1:
                continue
            assert _rel(crop1[b, k], crop0[b, k]) >= MARGIN * lr.MAP_RTOL, (b, p, k)
            if B <= 3:
                assert _rel(pool1[k], pool0[k]) >= MARGIN * lr.MAP_RTOL, (b, p, k)


def test_edge_maps_crop_record_mutations(edge_case):
    """Per-crop terms read from another crop's block records (two crops exchanged, or the stride
    over a crop's records forgotten) differ in every term by >= 100 x 2e-6; pooled terms that lose the
    records past 256 differ likewise."""
    shape, pred, gt, _, (s, n) = edge_case
    B = shape[0]
    bs, bn = lr.block_records(pred, gt)
    nbx = bs.shape[1]
    want = lr.per_crop(s, n)[0]
    pairs = [(b, b + 1) for b in range(B - 1)] + ([(0, B - 1)] if B > 2 else [])
    for a, b in pairs:
        for k in range(4):
            d = abs(float(want[a, k]) - float(want[b, k]))
            assert d >= MARGIN * lr.MAP_RTOL * max(abs(float(want[a, k])), abs(float(want[b, k]))), (a, b, k)
    if nbx > 1:  # crop b reading records [b, b + nbx) of the flat array
        fs, fn = bs.reshape(B * nbx, 4), bn.reshape(B * nbx, 4)
        for b in range(1, min(B, 4)):
            got = lr._ratio(fs[b:b + nbx].sum(0), fn[b:b + nbx].sum(0))
            for k in range(4):
                assert abs(float(got[k]) - float(want[b, k])) >= MARGIN * lr.MAP_RTOL * abs(float(want[b, k])), (b, k)
    if B * nbx > 256:
        fs, fn = bs.reshape(B * nbx, 4), bn.reshape(B * nbx, 4)
        got, full = lr._ratio(fs[:256].sum(0), fn[:256].sum(0)), lr.pooled(s, n)[0]
        for k in range(4):
            assert _rel(got[k], full[k]) >= MARGIN * lr.MAP_RTOL, k


def test_branch_maps_reach_their_branches():
    pred, gt = lr.branch_maps()
    loss, valid = lr.map_pixels(pred, gt)
    s, n = lr.map_terms(pred, gt)
    val, cnt = lr.pooled(s, n)
    assert int(cnt[0]) == 0 and float(val[0]) == 0.0  # xyz: +-0.0 everywhere
    assert torch.isfinite(val).all() and (cnt[1:] > 0).all()
    cap = -np.log(lr.EPS32)
    for k in (2, 3):
        assert abs(float(loss[k, 0, 4]) - cap) < 1e-9 and valid[k, 0, 4]  # probability underflows
        assert abs(float(loss[k, 1, 5]) + np.log1p(lr.EPS32)) < 1e-12 and valid[k, 1, 5]  # probability 1
        assert not valid[k, 0, 6] and not valid[k, 1, 7]  # labels -1 and C
    assert valid[1, 0, 1] and float(loss[1, 0, 1]) == 1.0  # zero predicted normal
    assert valid[1, 0, 2] and not valid[1, 1, 3]  # 1e-9 target valid, -0.0 target not
    # the f32 torch form would overflow without the max subtraction and gives NaN for the empty term
    assert not torch.isfinite(torch.exp(pred["region"][0, 0].flatten()[4]))
    assert torch.isnan(lo.map_loss(lo.l1, pred["xyz"], gt["xyz"]))
    _, cnt2 = lr.pooled(*lr.map_terms(*lr.branch_maps(empty_mask=True)))
    assert int(cnt2[3]) == 0 and int(cnt2[2]) == int(cnt[2])


@pytest.fixture(scope="module", params=POINT_P)
def point_case(request):
    P = request.param
    R, t, mp, tg = lr.edge_points(3, P, SYM3, seed=100 + P)
    ref = lr.points_ref(R, t, mp, tg, SYM3)
    r32 = lr.points_ref(R, t, mp, tg, SYM3, dtype=torch.float32)
    mc = lr.max_coord(R, t, mp, tg)
    return P, (R, t, mp, tg), ref, r32, mc


def test_edge_points_isolation(point_case):
    P, (R, t, mp, tg), ref, _, _ = point_case
    S, T = lr.special_indices(P)
    for b in (1, 2):
        pred = mp[b].double() @ R[b].double().T + t[b].double()
        for i in S:
            row_p = (pred[i] - tg[b].double()).norm(dim=1)  # prediction i to every target
            row_t = (tg[b, i].double() - pred).norm(dim=1)  # target i to every prediction
            for row in (row_p, row_t):
                j = int(row.argmin())
                assert j in T and row[j] < 0.95 * lr.STATION_D
                rest = row.clone()
                rest[j] = np.inf
                assert rest.min() >= 0.3 + row[j]


def test_edge_points_mutations(point_case):
    """Removing any one tile-edge candidate, or swapping the matching direction, moves the value the
    GPU test compares by >= 100 x that test's tolerance."""
    P, (R, t, mp, tg), ref, r32, mc = point_case
    tol_pose = float(lr.point_tol(ref["pose"].mean(), r32["pose"].mean(), mc))
    tol_adds = lr.point_tol(ref["adds"], r32["adds"], mc)
    # the direction: PoseLoss against ADD-S on the same symmetric crops
    for b in (1, 2) if P > 1 else ():  # (one point against one point has no direction)
        assert abs(float(ref["pose"][b] - ref["adds"][b])) / 3 >= MARGIN * tol_pose
        assert abs(float(ref["pose"][b] - ref["adds"][b])) >= MARGIN * float(tol_adds[b])
    if P < 3:
        return
    _, T = lr.special_indices(P)
    for b in (1, 2):
        for j in T:
            m = lr.points_ref(R[b:b + 1], t[b:b + 1], mp[b:b + 1], lr.drop_point(tg[b:b + 1], 0, j), [True],
                              terms=("pose",))
            d_pose = abs(float(m["pose"][0] - ref["pose"][b])) / 3  # one crop of the batch mean over 3
            assert d_pose >= MARGIN * tol_pose, (P, b, j, d_pose, tol_pose)
            m = lr.points_ref(R[b:b + 1], t[b:b + 1], lr.drop_point(mp[b:b + 1], 0, j), tg[b:b + 1], [True],
                              terms=("adds",))
            d_adds = abs(float(m["adds"][0] - ref["adds"][b]))
            assert d_adds >= MARGIN * float(tol_adds[b]), (P, b, j, d_adds, float(tol_adds[b]))


def test_empty_sym_list_is_not_class_zero():
    """The inputs of the sym=[] case: ADD and ADD-S of a class-0 crop differ by far more than the
    tolerance, so a kernel that read the placeholder [0] as a symmetric class would show."""
    R, t, mp, tg = lr.edge_points(2, 300, [True, True], seed=5)
    ref = lr.points_ref(R, t, mp, tg, [True, True])
    assert (ref["add"] - ref["adds"]).abs().min() > 1e-2
