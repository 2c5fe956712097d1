"""Batched Umeyama-RANSAC (krrn_umeyama_ransac_f32 / krrn_model_points_f32) on the GPU against the
results recorded from the reference's own estimateSimilarityTransform
(tests/golden/umeyama_scenes.npz) and against its numpy f64 restatement (tests/umeyama_ref.py) on
identical subsets. Every comparison is made only where the restatement's margins (threshold,
early stop, conditioning) show that a bit-different f64 evaluation must reach the same discrete
decisions; the tolerance on scale / R / t is the f32 output format's (values below 2 round within
1.2e-7; the f64 error is negligible at the asserted conditioning)."""
import os

import numpy as np
import pytest
import torch

import umeyama_ref as ur
from pose_estimation_amd import pose
from pose_estimation_amd.runtime import Plan, ptr
from pose_estimation_amd.umeyama import estimateSimilarityTransform

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umeyama_scenes.npz")
SCENES = ("exact", "tail", "long", "planar", "scaled", "fail")
TOL = 1e-6
EXT = np.array([0.067, 0.1276, 0.1175])
LFB = np.array([-0.0335, -0.0638, -0.0587])


def _rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _synth(seed, N, out_frac=0.0, noise=0.0, planar=False, scale=1.0):
    """LineMOD-sized model points under a random pose at ~0.9 m (f32 src / dst)."""
    rng = np.random.default_rng(seed)
    u = rng.random((N, 3)).astype(np.float32)
    if planar:
        u[:, 2] = np.float32(0.5)
    src = (u.astype(np.float64) * EXT + LFB).astype(np.float32)
    R = _rodrigues(rng.normal(size=3))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.1)])
    dst = scale * src.astype(np.float64) @ R.T + t
    if noise:
        dst += rng.normal(scale=noise, size=dst.shape)
    out = rng.random(N) < out_frac
    dst[out] = t + rng.uniform(-0.15, 0.15, size=(int(out.sum()), 3))
    return src, dst.astype(np.float32)


def _run(dev, src, dst, subsets):
    """src / dst [B, N, 3], subsets [B, H, 5] numpy -> dict of numpy results."""
    s, R, t, T, info = estimateSimilarityTransform(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
                                                   subsets=torch.from_numpy(subsets), return_info=True)
    torch.cuda.synchronize()
    out = dict(scale=s, R=R, t=t, T=T, **info)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, b, ref):
    assert np.array_equal(got["hyp_counts"][b], ref["counts"]), np.nonzero(got["hyp_counts"][b] != ref["counts"])
    assert int(got["best_hyp"][b]) == ref["best_hyp"]
    assert int(got["inliers"][b]) == ref["inliers"]
    assert np.array_equal(got["mask"][b].astype(bool), ref["mask"])
    es, eR, et = abs(got["scale"][b] - ref["scale"]), np.abs(got["R"][b] - ref["R"]).max(), \
        np.abs(got["t"][b] - ref["t"]).max()
    print(f"crop {b}: |s - s_ref| {es:.2e}  |R - R_ref| {eR:.2e}  |t - t_ref| {et:.2e} m")
    assert es <= TOL and eR <= TOL and et <= TOL, (es, eR, et)
    T = np.eye(4)
    T[:3, :3] = got["scale"][b] * got["R"][b]
    T[:3, 3] = got["t"][b]
    assert np.abs(got["T"][b] - T).max() <= 1e-6
    if ref["failed"]:
        assert got["scale"][b] == 1.0 and np.array_equal(got["R"][b], np.eye(3)) and np.all(got["t"][b] == 0)


@pytest.mark.parametrize("name", SCENES)
def test_fixture_parity(dev, name):
    """The recorded subsets through estimateSimilarityTransform: every hypothesis's count, the
    selection and the inlier count equal the restatement's; scale / R / t within 1e-6 of what the
    reference's own code returned; the fail scene reports failure."""
    z = np.load(GOLDEN)
    src, dst, sub = z[f"{name}_src"], z[f"{name}_dst"], z[f"{name}_subsets"]
    ref = ur.ransac(src, dst, sub)
    ur.check_conditions(ref)
    assert ref["failed"] == bool(z[f"{name}_failed"])
    got = _run(dev, src[None], dst[None], sub[None])
    _compare(got, 0, ref)
    assert abs(got["scale"][0] - float(z[f"{name}_scale"])) <= TOL
    assert np.abs(got["R"][0] - z[f"{name}_R"]).max() <= TOL
    assert np.abs(got["t"][0] - z[f"{name}_t"]).max() <= TOL
    if name == "fail":
        assert got["inliers"][0] == 0 and got["best_hyp"][0] == -1


def test_two_dim_input_is_one_crop(dev):
    z = np.load(GOLDEN)
    src, dst, sub = z["tail_src"], z["tail_dst"], z["tail_subsets"]
    s, R, t, T = estimateSimilarityTransform(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
                                             subsets=torch.from_numpy(sub))
    assert s.shape == (1,) and R.shape == (1, 3, 3) and t.shape == (1, 3) and T.shape == (1, 4, 4)
    assert abs(float(s[0]) - float(z["tail_scale"])) <= TOL


def test_smallest_problem(dev):
    """N = 5, H = 1, the sample is the whole set."""
    src, dst = _synth(11, 5)
    sub = np.arange(5, dtype=np.int32).reshape(1, 5)
    ref = ur.ransac(src, dst, sub)
    ur.check_conditions(ref)
    assert ref["inliers"] == 5
    _compare(_run(dev, src[None], dst[None], sub[None]), 0, ref)


def test_largest_problem(dev):
    """N = 4096, H = 128: 96 KiB of points in LDS (the opt-in above 64 KiB), 16 points per lane."""
    N = 4096
    src, dst = _synth(12, N, out_frac=0.3, noise=1e-3)
    sub = np.random.default_rng(12).integers(N, size=(128, 5)).astype(np.int32)
    ref = ur.ransac(src, dst, sub)
    ur.check_conditions(ref)
    assert not ref["failed"]
    _compare(_run(dev, src[None], dst[None], sub[None]), 0, ref)


def _mixed_batch():
    N = 257
    specs = [dict(out_frac=0.3, noise=1e-3), dict(out_frac=0.2, noise=1e-3, planar=True),
             dict(out_frac=0.2, noise=1e-3, scale=1.7), dict(out_frac=0.97, noise=2e-3), dict()]
    scenes = [_synth(20 + i, N, **sp) for i, sp in enumerate(specs)]
    src = np.stack([s for s, _ in scenes])
    dst = np.stack([d for _, d in scenes])
    sub = np.random.default_rng(20).integers(N, size=(5, 128, 5)).astype(np.int32)
    return src, dst, sub


@pytest.fixture(scope="module")
def mixed(dev):
    src, dst, sub = _mixed_batch()
    refs = [ur.ransac(src[b], dst[b], sub[b]) for b in range(5)]
    return src, dst, sub, refs, _run(dev, src, dst, sub)


def test_mixed_batch(mixed):
    """B = 5 at N = 257 (one point past a 256 block): outliers, planar, scaled, failing, exact."""
    src, dst, sub, refs, got = mixed
    assert [r["failed"] for r in refs] == [False, False, False, True, False]
    for b in range(5):
        ur.check_conditions(refs[b])
        _compare(got, b, refs[b])


def test_batch_invariance(dev, mixed):
    """Each crop of the B = 5 run alone at B = 1: bit-identical outputs."""
    src, dst, sub, _, got = mixed
    for b in range(5):
        one = _run(dev, src[b:b + 1], dst[b:b + 1], sub[b:b + 1])
        for k in ("scale", "R", "t", "inliers", "best_hyp", "hyp_counts", "mask"):
            assert np.array_equal(one[k][0:1].view(np.uint8), got[k][b:b + 1].view(np.uint8)), (b, k)


def test_all_duplicate_sample_counts_zero(dev):
    """A subset row of five identical indices has no scale (the reference gets NaN and no inliers):
    count 0, and the other rows still give a valid best."""
    N = 257
    src, dst = _synth(30, N, out_frac=0.2, noise=1e-3)
    sub = np.random.default_rng(30).integers(N, size=(16, 5)).astype(np.int32)
    sub[0] = 7
    sub[9] = 200
    ref = ur.ransac(src, dst, sub)
    assert not ref["margins"]["finite"] and ref["counts"][0] == 0 and ref["counts"][9] == 0
    ur.check_conditions(ref, allow_degenerate=True)
    assert not ref["failed"]
    _compare(_run(dev, src[None], dst[None], sub[None]), 0, ref)


def test_eager_and_plan_are_one_launch(dev):
    """estimateSimilarityTransform and a Plan built from the same step function (umeyama.ransac_step) on
    the same explicit subsets: one kernel through two host paths, so every output is bit-equal."""
    from pose_estimation_amd import umeyama
    B, N, H = 2, 300, 16
    scenes = [_synth(40, N, out_frac=0.3, noise=1e-3), _synth(41, N)]
    src = torch.from_numpy(np.stack([s for s, _ in scenes])).to(dev)
    dst = torch.from_numpy(np.stack([d for _, d in scenes])).to(dev)
    sub = torch.from_numpy(np.random.default_rng(40).integers(N, size=(B, H, 5)).astype(np.int32))
    scale, R, t, _, info = estimateSimilarityTransform(src, dst, subsets=sub, return_info=True)
    plan = Plan(dev)
    ps, pR, pt, pinfo = umeyama.ransac_step(plan, src, dst, B, N, H, info["subsets"])
    assert [op.name for op in plan.ops] == ["krrn_umeyama_ransac_f32"]
    plan.run({})
    torch.cuda.synchronize()
    assert torch.equal(ps, scale) and torch.equal(pR, R) and torch.equal(pt, t)
    for k in ("inliers", "best_hyp", "hyp_counts", "mask"):
        assert torch.equal(pinfo[k], info[k]), k
    assert (info["inliers"] > 0).all()


def _pose_scene(B, N, S, seed, outlier_frac=0.1):
    """test_gpu_pnp._scene's xyz maps plus the cloud of the same pose: cloud = R obj + t."""
    from test_gpu_pnp import _scene
    xyz, data, Rgt, tgt = _scene(B, N, S, seed, outlier_frac=0.0)
    rng = np.random.default_rng(seed + 1000)
    cloud = np.zeros((B, N, 3), np.float32)
    srcs = []
    for b in range(B):
        pix = data["choose"][b, 0]
        u = xyz[b].reshape(3, -1)[:, pix].double().t()
        obj = (u * data["extent"][b] + data["lfborder"][b]).float()
        srcs.append(obj)
        c = obj.double().numpy() @ Rgt[b].T + tgt[b]
        out = rng.random(N) < outlier_frac
        c[out] = tgt[b] + rng.uniform(-0.15, 0.15, size=(int(out.sum()), 3))
        cloud[b] = c
    data["cloud"] = torch.from_numpy(cloud)
    return xyz, data, Rgt, tgt, torch.stack(srcs)


def test_get_pose_umeyama_known_answer(dev):
    B, N, S = 4, 1000, 60
    xyz, data, Rgt, tgt, src = _pose_scene(B, N, S, 3)
    pose._seeds.clear()  # the device draws start from seed 0 whatever ran before
    R, t, info = pose.get_pose_umeyama({"xyz": xyz.to(dev)}, data, return_info=True)
    torch.cuda.synchronize()
    # the model points equal the torch f64 -> f32 expression bit for bit
    assert np.array_equal(info["src"].cpu().numpy().view(np.uint32), src.numpy().view(np.uint32))
    eR, et = np.abs(R.cpu().numpy() - Rgt).max(), np.abs(t.cpu().numpy() - tgt).max()
    es = np.abs(info["scale"].cpu().numpy() - 1.0).max()
    print(f"|R - R_gt| {eR:.2e}  |t - t_gt| {et:.2e} m  |s - 1| {es:.2e}")
    assert eR < 1e-4 and et < 1e-4 and es < 1e-4
    assert (info["inliers"].cpu().numpy() >= 0.85 * N).all()
    sub = info["subsets"].cpu().numpy()
    assert sub.shape == (B, 128, 5) and sub.min() >= 0 and sub.max() < N
    assert all(len(set(row)) == 5 for row in sub.reshape(-1, 5).tolist())  # device draws are distinct
    # explicit subsets: the restatement's decisions on the same samples
    R2, t2, info2 = pose.get_pose_umeyama({"xyz": xyz.to(dev)}, data, subsets=info["subsets"], return_info=True)
    assert torch.equal(R2, R) and torch.equal(t2, t)
    ref = ur.ransac(src[0].numpy(), data["cloud"][0].numpy(), sub[0])
    ur.check_conditions(ref)
    assert np.array_equal(info["hyp_counts"][0].cpu().numpy(), ref["counts"])
    assert int(info["best_hyp"][0]) == ref["best_hyp"]


def test_plan_and_graph_replay(dev):
    """add_umeyama_ops in a plan: two eager runs and one hipGraph replay (one straight-line capture,
    no side streams) from the same seed give identical bits."""
    B, N, S = 3, 300, 40
    xyz, data, Rgt, tgt, _ = _pose_scene(B, N, S, 5)
    xyz_d = xyz.to(dev).contiguous()
    choose = data["choose"].reshape(B, N).to(dev)
    cloud = data["cloud"].to(dev).contiguous()
    ext = data["extent"].to(dev).double().contiguous()
    lfb = data["lfborder"].to(dev).double().contiguous()
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    plan = Plan(dev)
    R, t, inl, aux = pose.add_umeyama_ops(plan, xyz_d, choose, cloud, B, N, ext, lfb, seed)
    plan.add("krrn_rng_advance", ptr(seed))
    outs = (R, t, inl, aux["scale"], aux["subsets"], aux["hyp_counts"], aux["best_hyp"], aux["mask"])

    def snap():
        torch.cuda.synchronize()
        return [o.clone() for o in outs]

    def clear():
        seed.zero_()
        for o in outs:
            o.zero_()

    plan.run({})
    first = snap()
    assert int(seed.item()) == 1
    clear()
    plan.run({})
    second = snap()
    clear()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.run({})
    torch.cuda.current_stream().wait_stream(s)
    clear()
    g.replay()
    third = snap()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert np.abs(first[0].cpu().numpy() - Rgt).max() < 1e-4
    assert np.abs(first[1].cpu().numpy() - tgt).max() < 1e-4
    assert (first[2] > 0).all()


class _GroundTruthMaps:
    """Stands in for the network in eval_records: the xyz map a perfect network would predict for the
    batch's cloud under its ground-truth pose (noiseless crops), so the records show what the pose
    solver makes of it. The batch is found by its cloud tensor."""
    return_views = False

    def __init__(self, seen):
        self.seen = seen

    def __call__(self, img, cloud, choose, cls_id, opt_pose=True):
        d = self.seen[cloud.data_ptr()]
        B, N = cloud.shape[0], cloud.shape[1]
        S = img.shape[-1]
        Rg, tg = d["target_r"].double(), d["target_t"].double().reshape(B, 1, 3)
        p = (cloud.double() - tg) @ Rg  # R^T (c - t), row vectors
        u = ((p - d["lfborder"].double().reshape(B, 1, 3)) / d["extent"].double().reshape(B, 1, 3)).float()
        xyz = torch.zeros((B, 3, S * S), dtype=torch.float32, device=cloud.device)
        xyz.scatter_(2, choose.reshape(B, 1, N).expand(B, 3, N), u.transpose(1, 2).contiguous())
        return {"xyz": xyz.view(B, 3, S, S), "pred_t": d["target_t"].reshape(B, 3).clone()}


def test_eval_records_umeyama(dev, tmp_path):
    """eval_records(pose_solver="umeyama") on the synthetic LineMOD tree: finite records, base ADD
    below the diameter on noiseless crops."""
    from linemod_tree import write_tree
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import _R, eval_records
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
    rec = eval_records(_GroundTruthMaps(seen), ds, buckets, 4, dev, with_loss=False, pose_solver="umeyama").numpy()
    assert rec.shape[0] == len(ds) == 4
    assert np.isfinite(rec).all()
    dia = np.array([ds.diameter[int(c)] for c in rec[:, _R["cls"]]])
    print("add_b", rec[:, _R["add_b"]], "r_b", rec[:, _R["r_b"]], "t_b", rec[:, _R["t_b"]])
    assert (rec[:, _R["add_b"]] < dia).all()
