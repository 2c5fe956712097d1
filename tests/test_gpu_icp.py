"""Batched ICP pose refinement (krrn_icp_refine_f32 through icp.refine / pose.refine_pose_icp /
pose.add_icp_ops / evaluate.eval_records(refine="icp")) on the GPU against its numpy f64 restatement
(tests/icp_ref.py) on the shared scene family. The discrete results (passes, pairs, status, every
nearest-neighbour index) are compared exactly, which the restatement's margins license
(icp_ref.check_conditions: a bit-different f64 evaluation reaches the same decisions); R / t / rmse
within the f32 output format's 1e-6 (tests/test_gpu_umeyama.py's TOL: values below 2 round within
1.2e-7, the f64 differences are far below that)."""
import numpy as np
import pytest
import torch

import icp_ref as ir
from pose_estimation_amd import icp, pose
from pose_estimation_amd.runtime import Plan

pytestmark = pytest.mark.gpu

TOL = 1e-6
KEYS = ("R", "t", "rmse", "passes", "pairs", "status", "nn_idx")


def _run(dev, scs, max_dist, with_info=True, **kw):
    """Scenes of one shape as a batch through icp.refine -> dict of numpy results."""
    g = lambda k: torch.from_numpy(np.stack([s[k] for s in scs])).to(dev)  # noqa: E731
    md = torch.from_numpy(np.asarray(max_dist, np.float32)).to(dev) if np.ndim(max_dist) else float(max_dist)
    out = icp.refine(g("R0"), g("t0"), g("cloud"), g("model"), md, return_info=with_info, **kw)
    torch.cuda.synchronize()
    res = dict(R=out[0], t=out[1], **(out[2] if with_info else {}))
    return {k: v.cpu().numpy() for k, v in res.items() if v is not None}


def _compare(got, b, ref, tag):
    assert int(got["passes"][b]) == ref["passes"], (tag, got["passes"][b], ref["passes"])
    assert int(got["pairs"][b]) == ref["pairs"], (tag, got["pairs"][b], ref["pairs"])
    assert int(got["status"][b]) == ref["status"], (tag, got["status"][b], ref["status"])
    assert np.array_equal(got["nn_idx"][b], ref["nn_idx"]), (tag, np.nonzero(got["nn_idx"][b] != ref["nn_idx"]))
    eR, et = np.abs(got["R"][b] - ref["R"]).max(), np.abs(got["t"][b] - ref["t"]).max()
    er = 0.0 if np.isinf(ref["rmse"]) and got["rmse"][b] == np.inf else abs(float(got["rmse"][b]) - ref["rmse"])
    print(f"{tag}: passes {ref['passes']} pairs {ref['pairs']} status {icp.STATUS[ref['status']]}  "
          f"|R - R_ref| {eR:.2e}  |t - t_ref| {et:.2e} m  |rmse - rmse_ref| {er:.2e} m")
    assert eR <= TOL and et <= TOL and er <= TOL, (tag, eR, et, er)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", ir.SCENES)
def test_scene_parity(dev, name):
    sc, ref = ir.scene(name), ir.reference(name)
    ir.check_conditions(ref)
    got = _run(dev, [sc], sc["max_dist"], **sc["kw"])
    _compare(got, 0, ref, name)
    if name == "far":
        assert got["pairs"][0] == 0 and got["rmse"][0] == np.inf and got["status"][0] == ir.STARVED
        assert np.array_equal(_bits(got["R"][0]), _bits(sc["R0"])) and np.array_equal(_bits(got["t"][0]), _bits(sc["t0"]))
    if name == "exact":
        eR, et = np.abs(got["R"][0] - sc["R_gt"]).max(), np.abs(got["t"][0] - sc["t_gt"]).max()
        print(f"exact: |R - R_gt| {eR:.2e}  |t - t_gt| {et:.2e} m")
        assert eR <= TOL and et <= TOL
    if name == "dup":
        assert got["nn_idx"][0].max() < 65
        one = _run(dev, [dict(sc, model=sc["model65"])], sc["max_dist"])
        for k in KEYS:
            assert np.array_equal(_bits(one[k]), _bits(got[k])), k


def test_two_dim_input_is_one_crop(dev):
    sc = ir.scene("odd")
    R, t = icp.refine(*(torch.from_numpy(sc[k].copy()).to(dev) for k in ("R0", "t0", "cloud", "model")), sc["max_dist"])
    assert R.shape == (1, 3, 3) and t.shape == (1, 3)
    assert np.abs(R[0].cpu().numpy() - ir.reference("odd")["R"]).max() <= TOL
    with pytest.raises(ValueError):
        icp.refine(torch.zeros(2, 3, 3, device=dev), torch.zeros(2, 3, device=dev), torch.zeros(3, 8, 3, device=dev),
                   torch.zeros(3, 8, 3, device=dev), 0.02)
    with pytest.raises(ValueError):
        icp.refine(torch.zeros(2, 3, 3, device=dev), torch.zeros(2, 3, device=dev), torch.zeros(2, 8, 3, device=dev),
                   torch.zeros(2, 8, 3, device=dev), torch.zeros(3, device=dev))


@pytest.fixture(scope="module")
def mixed(dev):
    scs, md = ir.mixed_batch()
    refs = [ir.icp(s["R0"], s["t0"], s["cloud"], s["model"], m) for s, m in zip(scs, md)]
    return scs, md, refs, _run(dev, scs, md)


def test_mixed_batch(mixed):
    """B = 5 at N = 257 / M = 65 with a max_dist per crop: a far crop and an early stop among them."""
    scs, md, refs, got = mixed
    assert refs[2]["status"] == ir.STARVED and refs[2]["passes"] == 1
    assert refs[3]["passes"] < refs[0]["passes"]
    for b in range(5):
        ir.check_conditions(refs[b])
        _compare(got, b, refs[b], f"crop {b}")


def test_batch_invariance(dev, mixed):
    """Each crop of the B = 5 run alone at B = 1: bit-identical outputs."""
    scs, md, _, got = mixed
    for b in range(5):
        one = _run(dev, scs[b:b + 1], md[b:b + 1])
        for k in KEYS:
            assert np.array_equal(_bits(one[k][0]), _bits(got[k][b])), (b, k)


def test_max_iter_zero_scores_the_input(dev):
    """One scoring pass: the pose comes back bit for bit, pairs / rmse / nn_idx describe it."""
    sc = ir.scene("odd")
    ref = ir.icp(sc["R0"], sc["t0"], sc["cloud"], sc["model"], sc["max_dist"], max_iter=0)
    ir.check_conditions(ref)
    assert ref["passes"] == 1 and ref["status"] == ir.MAX_ITER_HIT
    got = _run(dev, [sc], sc["max_dist"], max_iter=0)
    _compare(got, 0, ref, "max_iter 0")
    assert np.array_equal(_bits(got["R"][0]), _bits(sc["R0"])) and np.array_equal(_bits(got["t"][0]), _bits(sc["t0"]))


def test_non_finite_start_is_starved(dev):
    sc = dict(ir.scene("odd"))
    sc["R0"] = sc["R0"].copy()
    sc["R0"][1, 2] = np.nan
    got = _run(dev, [sc], sc["max_dist"])
    assert got["status"][0] == ir.STARVED and got["passes"][0] == 1 and got["pairs"][0] == 0
    assert got["rmse"][0] == np.inf and (got["nn_idx"][0] == -1).all()
    assert np.array_equal(_bits(got["R"][0]), _bits(sc["R0"])) and np.array_equal(_bits(got["t"][0]), _bits(sc["t0"]))


def test_null_nn_idx(dev):
    """Without the optional nn_idx buffer (return_info=False passes a null pointer): the same pose bits."""
    sc = ir.scene("outl")
    full = _run(dev, [sc], sc["max_dist"])
    bare = _run(dev, [sc], sc["max_dist"], with_info=False)
    assert np.array_equal(_bits(full["R"]), _bits(bare["R"])) and np.array_equal(_bits(full["t"]), _bits(bare["t"]))
    g = lambda k: torch.from_numpy(sc[k][None].copy()).to(dev)  # noqa: E731
    _, _, info = icp.solve(g("R0"), g("t0"), g("cloud"), g("model"), icp.dist_tensor(sc["max_dist"], 1, dev),
                           with_nn=False)
    torch.cuda.synchronize()
    assert info["nn_idx"] is None and int(info["pairs"][0]) == int(full["pairs"][0])


def test_plan_and_graph_replay(dev):
    """add_icp_ops in a plan, captured and replayed twice: both replays bit-equal to the eager call."""
    scs, md = ir.mixed_batch()
    B, N, M = 5, 257, 65
    g = lambda k: torch.from_numpy(np.stack([s[k] for s in scs])).to(dev).contiguous()  # noqa: E731
    R0, t0, cloud, model, mdt = g("R0"), g("t0"), g("cloud"), g("model"), torch.from_numpy(md).to(dev)
    eR, et, einfo = icp.refine(R0, t0, cloud, model, mdt, return_info=True)
    eager = [eR, et] + [einfo[k] for k in ("passes", "pairs", "rmse", "status", "nn_idx")]
    plan = Plan(dev)
    R, t, info = pose.add_icp_ops(plan, R0, t0, cloud, model, mdt, B, N, M)
    outs = [R, t] + [info[k] for k in ("passes", "pairs", "rmse", "status", "nn_idx")]

    def snap():
        torch.cuda.synchronize()
        return [o.clone() for o in outs]

    def clear():
        for o in outs:
            o.zero_()

    plan.run({})
    first = snap()
    clear()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            plan.run({})
    torch.cuda.current_stream().wait_stream(s)
    clear()
    graph.replay()
    second = snap()
    clear()
    graph.replay()
    third = snap()
    for e, a, b, c in zip(eager, first, second, third):
        assert torch.equal(e, a) and torch.equal(e, b) and torch.equal(e, c)


def _add(R, t, data):
    """ADD of (R, t) per crop against the batch's target points (f64, on the host)."""
    mp = data["model_points"].double().cpu()
    pred = mp @ R.double().cpu().transpose(1, 2) + t.double().cpu().reshape(-1, 1, 3)
    return (pred - data["target"].double().cpu()).norm(dim=2).mean(dim=1).numpy()


def test_refine_pose_icp_on_synthetic_batch(dev):
    """pose.refine_pose_icp on a synthetic.make_batch batch from the ground truth turned by 3 degrees and
    moved by 5 mm: ADD falls for every crop. The generator's depth is a smooth bump that has nothing to do
    with its model points, so the cloud is replaced by N of the batch's own `target` points (the model
    under the ground-truth pose) with 1 mm noise; everything else is the batch as generated."""
    from pose_estimation_amd.synthetic import make_batch
    B, N = 4, 500
    data = make_batch(B, 64, N, seed=3)
    rng = np.random.default_rng(3)
    pick = np.stack([rng.choice(data["target"].shape[1], N, replace=False) for _ in range(B)])
    cloud = data["target"].numpy()[np.arange(B)[:, None], pick].astype(np.float64)
    data["cloud"] = torch.from_numpy((cloud + rng.normal(scale=1e-3, size=cloud.shape)).astype(np.float32))
    Rg, tg = data["target_r"].double().numpy(), data["target_t"].double().numpy()
    R0 = np.stack([ir.rodrigues(rng.normal(size=3), 3.0) @ Rg[b] for b in range(B)]).astype(np.float32)
    d = rng.normal(size=(B, 3))
    t0 = (tg + 0.005 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    R0, t0 = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev)
    dia = torch.full((B,), 0.15, device=dev)  # about the cat's diameter: max_dist 15 mm
    R, t, info = pose.refine_pose_icp(R0, t0, data, diameter=dia, return_info=True)
    torch.cuda.synchronize()
    before, after = _add(R0, t0, data), _add(R, t, data)
    print("ADD before", before, "after", after, "passes", info["passes"].tolist(), "pairs", info["pairs"].tolist())
    assert (after < before).all()
    R2, t2 = pose.refine_pose_icp(R0, t0, data, max_dist=icp.DIST_FRAC * 0.15)  # the same max_dist, given directly
    assert torch.equal(R2, R) and torch.equal(t2, t)
    with pytest.raises(ValueError, match="diameter"):
        pose.refine_pose_icp(R0, t0, data)


def test_eval_records_icp(dev, tmp_path):
    """eval_records(refine="icp") on the synthetic LineMOD tree with the ground-truth-map stand-in for the
    network: finite records; add_b is add_metric of refine_pose_icp applied to get_pose's own output under
    the same host and device RNG state; refine=None gives the records of a call without the keyword."""
    from linemod_tree import write_tree
    from test_gpu_umeyama import _GroundTruthMaps
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import _R, _batches, eval_records
    from pose_estimation_amd.metric import add_metric
    write_tree(str(tmp_path), objs=(6,), per_obj=4, sizes=(80, 120))
    ds = PoseDataset("test", 500, False, str(tmp_path), 0.0, 8, cls_type="cat")
    seen = {}
    inner = ds.batch

    def batch(indices, device):
        d = inner(indices, device)
        seen[d["cloud"].data_ptr()] = d
        return d

    ds.batch = batch
    buckets = {}
    for i in range(len(ds)):
        buckets.setdefault(ds.crop_size(i), []).append(i)

    def run(**kw):
        seen.clear()
        ds._calls = 0           # the inputs' point draws are numbered by call
        pose._seeds.clear()     # the device draws of get_pose start from seed 0
        torch.manual_seed(11)   # get_pose's host draws
        rec = eval_records(_GroundTruthMaps(seen), ds, buckets, 4, dev, with_loss=False, **kw).numpy()
        return rec, list(seen.values())

    rec, datas = run(refine="icp")
    assert rec.shape[0] == len(ds) == 4 and np.isfinite(rec).all()
    print("add_b", rec[:, _R["add_b"]], "add_f", rec[:, _R["add_f"]], "r_b", rec[:, _R["r_b"]])
    # the same steps by hand, batch by batch in the order eval_records takes them
    pose._seeds.clear()
    torch.manual_seed(11)
    model = _GroundTruthMaps({d["cloud"].data_ptr(): d for d in datas})
    want_b, want_f = [], []
    for d, (S, idx) in zip(datas, _batches(buckets, 4)):
        B = len(idx)
        pred = model(d["img_croped"], d["cloud"], d["choose"], d["cls_id"])
        R, t = pose.get_pose({"xyz": pred["xyz"]}, d)
        dia = torch.tensor([ds.diameter[int(c)] for c in d["cls_id"].reshape(B).tolist()], dtype=torch.float32,
                           device=dev)
        Rb, tb = pose.refine_pose_icp(R, t.reshape(B, 3), d, diameter=dia)
        Rf, tf = pose.refine_pose_icp(R, pred["pred_t"].reshape(B, 3), d, diameter=dia)
        want_b.append(add_metric(Rb, tb, d["model_points"], d["target"], d["cls_id"], []))
        want_f.append(add_metric(Rf, tf, d["model_points"], d["target"], d["cls_id"], []))
    assert np.array_equal(rec[:, _R["add_b"]], torch.cat(want_b).cpu().numpy())
    assert np.array_equal(rec[:, _R["add_f"]], torch.cat(want_f).cpu().numpy())
    plain, _ = run()
    none, _ = run(refine=None)
    assert np.array_equal(plain.view(np.uint8), none.view(np.uint8))
