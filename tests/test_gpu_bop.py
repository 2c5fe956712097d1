"""The BOP-19 pose errors on the GPU (krrn_bop_vsd_f32 / krrn_bop_mssd_mspd_f32 through bop.vsd, bop.mssd_mspd,
bop.bop_errors and evaluate.test_epoch(bop=True)) against their numpy f64 restatement (tests/bop_ref.py).

VSD: the integer counts (union, inter, step_k) are compared exactly, which the restatement's margins license
(bop_ref.check_conditions: no undecided pixel in any scene); e_vsd is one f64 division of those integers, so bit
equality is expected and asserted. Scenes (frame, faces, what it pins): tetra (480 x 640, 4), layers (4: occlusion
inside the mesh), degenerate (87: skipped faces), sphere (1280: five face chunks), gross (80: inter = 0), empty_obs
(320: an all-zero observed frame), small (90 x 120, 320: partial tiles, the object cut by two frame borders), mixed
(B = 5 over one concatenated mesh, one empty face range).

MSSD / MSPD: kernel and restatement evaluate the same IEEE expressions (f64 +, *, /, sqrt are correctly rounded on
both sides and the build has no FMA contraction), so they are expected to agree bit for bit. Measured on MI355X
over the nine (V, NS) cases below: largest relative difference 0. MS_TOL is therefore ten times the smallest
difference that could be observed at all, one ulp (2^-52)."""
import numpy as np
import pytest
import torch

import bop_ref as br
import raster_ref as rr
from pose_estimation_amd import bop

pytestmark = pytest.mark.gpu

MS_TOL = 10 * 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt))


def _vsd(dev, verts, faces, face_range, crops, frames, frame_idx):
    """bop.vsd over `crops` (scene dicts: their poses, K4, diameter); the rest as given."""
    out = bop.vsd(_t(verts, np.float32).to(dev), _t(faces, np.int32).reshape(-1, 3).to(dev), _t(face_range, np.int32),
                  _t(np.stack([c["R_est"] for c in crops]), np.float64), _t(np.stack([c["t_est"] for c in crops]), np.float64),
                  _t(np.stack([c["R_gt"] for c in crops]), np.float64), _t(np.stack([c["t_gt"] for c in crops]), np.float64),
                  _t(np.stack([c["K4"] for c in crops]), np.float32), _t(frames, np.float32).to(dev),
                  _t(frame_idx, np.int32), _t([c["diameter"] for c in crops], np.float64), br.DEPTH_SCALE, br.DELTA, br.TAUS)
    torch.cuda.synchronize()
    return out["counts"].cpu().numpy(), out["e_vsd"].cpu().numpy()


def _scene_vsd(dev, sc, frame_idx=0, face_range=None):
    fr = [[0, len(sc["faces"])]] if face_range is None else face_range
    return _vsd(dev, sc["verts"], sc["faces"], fr, [sc], sc["depth"][None], [frame_idx])


def _check(tag, counts, e, ref):
    rel = np.abs(e - ref["e_vsd"]) / np.maximum(np.abs(ref["e_vsd"]), 1e-300)
    print(f"{tag}: counts {counts.tolist()}  e_vsd {np.round(e, 4).tolist()}  max rel diff {rel.max():.1e}  "
          f"bit-equal {np.array_equal(_bits(e), _bits(ref['e_vsd']))}")
    assert np.array_equal(counts, ref["counts"]), (tag, counts.tolist(), ref["counts"].tolist())
    assert rel.max() <= 1e-15, (tag, rel.max())
    assert np.array_equal(_bits(e), _bits(ref["e_vsd"])), tag


@pytest.mark.parametrize("name", br.SCENES)
def test_vsd_scene_parity(dev, name):
    sc, ref = br.scene(name), br.reference(name)
    br.check_conditions(ref)
    counts, e = _scene_vsd(dev, sc)
    _check(name, counts[0], e[0], ref)


def test_vsd_known_answers_and_guards(dev):
    sc = br.scene("tetra")
    same = dict(sc, R_est=sc["R_gt"], t_est=sc["t_gt"])
    counts, e = _scene_vsd(dev, same)                            # est = GT
    ref = br.scene_vsd(same)
    assert counts[0, 0] == counts[0, 1] == int(ref["v_gt"].sum()) > 0 and not counts[0, 2:].any() and not e.any()
    for fi in (-1, 1, 7):                                        # a frame index outside [0, F): all-zero observed depth
        counts, e = _scene_vsd(dev, sc, frame_idx=fi)
        _check(f"frame {fi}", counts[0], e[0], br.scene_vsd(sc, depth=np.zeros_like(sc["depth"])))
    for bad in ([[0, 0]], [[-1, 4]], [[0, -4]], [[5, 4]]):       # an empty or bad face range: union = 0
        counts, e = _scene_vsd(dev, sc, face_range=bad)
        assert not counts.any() and (e == 1.0).all(), bad
    counts, e = _scene_vsd(dev, sc, face_range=[[2, 100]])       # cut at Ftot: faces 2 and 3
    _check("cut range", counts[0], e[0], br.scene_vsd(sc, faces=sc["faces"][2:]))


def test_vsd_mixed_batch_invariance(dev):
    """Five crops over one concatenated mesh with per-crop poses, frames and diameters: each equals its own
    reference and its single-crop launch bit for bit, also with crops and frame indices permuted together."""
    bt, crops, frames = br.mixed()
    B = rr.MIXED_B
    counts, e = _vsd(dev, bt["verts"], bt["faces"], bt["face_range"], crops, frames, list(range(B)))
    for b in range(B):
        ref = br.mixed_reference(b)
        br.check_conditions(ref)
        _check(f"mixed[{b}]", counts[b], e[b], ref)
        c1, e1 = _vsd(dev, bt["verts"], bt["faces"], bt["face_range"][b:b + 1], [crops[b]], frames, [b])
        assert np.array_equal(c1[0], counts[b]) and np.array_equal(_bits(e1[0]), _bits(e[b])), b
    assert not counts[3].any() and (e[3] == 1.0).all()           # the crop with face count 0
    perm = [3, 0, 4, 2, 1]
    cp, ep = _vsd(dev, bt["verts"], bt["faces"], bt["face_range"][perm], [crops[b] for b in perm], frames, perm)
    assert np.array_equal(cp, counts[perm]) and np.array_equal(_bits(ep), _bits(e[perm]))


def _ms_cases():
    """(verts, syms, est pose, GT pose) for V in {4, 162, 642} x NS in {1, 2, 315}: the estimate is the GT pose
    composed with one symmetry of the set, then perturbed, so that the arg-min is not the identity."""
    rng = np.random.default_rng(9)
    tet, S2 = br.sym_tetra()
    meshes = [tet, rr.icosphere(2, 0.04)[0].astype(np.float32) * np.float32([1.0, 0.8, 1.2]),
              rr.icosphere(3, 0.05)[0].astype(np.float32) * np.float32([0.7, 1.1, 1.0])]
    sets = [bop.symmetry_set(), S2, bop.symmetry_set(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}])]
    cases = []
    for v in meshes:
        for S in sets:
            k = (len(S) * 2) // 3
            R_gt, t_gt = rr.rotation(rng), rr._centre_t(rng.uniform(0.5, 1.0), rng.uniform(100, 500), rng.uniform(100, 400))
            R_est, t_est = br.perturbed(rng, R_gt @ S[k, :9].reshape(3, 3), R_gt @ S[k, 9:] + t_gt, deg=1.0, mm=2.0)
            cases.append(dict(verts=v, syms=S, R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt))
    return cases


def test_mssd_mspd_parity(dev):
    cases = _ms_cases()
    assert sorted({len(c["verts"]) for c in cases}) == [4, 162, 642]
    assert sorted({len(c["syms"]) for c in cases}) == [1, 2, 315]
    verts = np.concatenate([c["verts"] for c in cases])
    syms = np.concatenate([c["syms"] for c in cases])
    voff = np.cumsum([0] + [len(c["verts"]) for c in cases])
    soff = np.cumsum([0] + [len(c["syms"]) for c in cases])
    vr = [[int(voff[i]), len(c["verts"])] for i, c in enumerate(cases)] + [[0, 0], [0, 4], [-3, 4]]
    sr = [[int(soff[i]), len(c["syms"])] for i, c in enumerate(cases)] + [[0, 1], [0, 0], [0, 1]]
    pad = [cases[0]] * 3                                         # three crops with an empty vertex / symmetry range
    st = lambda k, dt: _t(np.stack([c[k] for c in cases + pad]), dt)  # noqa: E731
    K4 = np.tile(np.asarray(rr.LM_K4, np.float32), (len(vr), 1))
    out = bop.mssd_mspd(_t(verts, np.float32).to(dev), _t(vr, np.int32), st("R_est", np.float64), st("t_est", np.float64),
                        st("R_gt", np.float64), st("t_gt", np.float64), _t(K4, np.float32), _t(syms, np.float64),
                        _t(sr, np.int32))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    worst = 0.0
    for i, c in enumerate(cases):
        m3, m2, i3, i2, per3, per2 = br.mssd_mspd(c["verts"], c["R_est"], c["t_est"], c["R_gt"], c["t_gt"], rr.LM_K4, c["syms"])
        r3, r2 = abs(got["mssd"][i] - m3) / m3, abs(got["mspd"][i] - m2) / m2
        worst = max(worst, r3, r2)
        print(f"V {len(c['verts'])} NS {len(c['syms'])}: mssd {got['mssd'][i]:.6e} m (rel diff {r3:.1e}, sym {i3})  "
              f"mspd {got['mspd'][i]:.6e} px (rel diff {r2:.1e}, sym {i2})")
        assert r3 <= MS_TOL and r2 <= MS_TOL, (i, r3, r2)
        for per, ref_i, got_i in ((per3, i3, got["sym_idx"][i, 0]), (per2, i2, got["sym_idx"][i, 1])):
            two = np.sort(per)[:2]
            if len(per) == 1 or (two[1] - two[0]) > MS_TOL * two[1]:
                assert got_i == ref_i, (i, got_i, ref_i)
        if len(c["syms"]) == 2:
            assert i3 == 1                                       # the symmetry the estimate was built from
    print(f"largest relative difference {worst:.2e} (MS_TOL {MS_TOL:.2e})")
    n = len(cases)
    assert np.isposinf(got["mssd"][n:]).all() and np.isposinf(got["mspd"][n:]).all() and (got["sym_idx"][n:] == -1).all()


# ------------------------------------------------------------------------------------------- dataset, epoch

TODAY = {"img_croped", "choose", "cloud", "x_map_choosed", "y_map_choosed", "point_mask", "mask_count", "cls_id",
         "intrinsic", "extent", "lfborder", "bbox", "target_r", "target_t", "model_points", "target"}
BOP_KEYS = {"bop_depth", "bop_frame", "bop_face_range", "bop_vert_range", "bop_sym_range"}
AR_KEYS = {"AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "count"}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A 3-frame LineMOD-layout tree whose PLY has faces (tests/mesh_tree.py; tests/linemod_tree.py's PLYs have
    none): one object, crop sizes 40 / 80 / 40."""
    import mesh_tree
    root = str(tmp_path_factory.mktemp("bop_tree"))
    return root, mesh_tree.write_tree(root, objs=(6,), per_obj=(3,))


def _dataset(root, **kw):
    from pose_estimation_amd.dataset import PoseDataset
    return PoseDataset("test", 500, False, root, 0.0, 8, cls_type="cat", n_model_pts=150, **kw)


def test_bop_errors_with_gt_pose(dev, tree):
    from pose_estimation_amd.evaluate import _batches
    root, w = tree
    ds = _dataset(root, meshes=True)
    assert len(ds) == 3
    buckets = {}
    for i in range(len(ds)):
        buckets.setdefault(ds.crop_size(i), []).append(i)
    T = len(bop.TAUS)
    rec = np.zeros((len(ds), len(bop.BOP_REC)))
    o = 0
    for S, idx in _batches(buckets, 2):
        assert set(ds.batch(idx, dev)) == TODAY                  # the default keys are unchanged
        data = ds.batch(idx, dev, bop=True)
        assert set(data) == TODAY | BOP_KEYS
        assert tuple(data["bop_depth"].shape) == (len(idx), rr.H, rr.W) and data["bop_frame"].tolist() == list(range(len(idx)))
        assert data["bop_face_range"].tolist() == [[0, 320]] * len(idx) and data["bop_sym_range"].tolist() == [[0, 1]] * len(idx)
        err = bop.bop_errors(data["target_r"], data["target_t"], data, ds)   # pred = GT
        torch.cuda.synchronize()
        assert tuple(err["vsd"].shape) == (len(idx), T) and err["vsd"].dtype == torch.float64
        assert not err["vsd"].any() and not err["mssd"].any() and not err["mspd"].any()
        # and off by 3 cm along the optical axis (a third of the 6 cm object): every error is large
        far = bop.bop_errors(data["target_r"], data["target_t"] + torch.tensor([0.0, 0.0, 0.03], device=dev), data, ds)
        assert (far["vsd"][:, 0] > 0.9).all() and ((far["mssd"] - 0.03).abs() < 1e-6).all() and (far["mspd"] > 0).all()
        n = len(idx)
        rec[o:o + n, 0], rec[o:o + n, -1] = idx, 1.0
        rec[o:o + n, 2:2 + T] = err["vsd"].cpu().numpy()
        rec[o:o + n, 2 + T], rec[o:o + n, 3 + T] = err["mssd"].cpu().numpy(), err["mspd"].cpu().numpy()
        o += n
    res = bop.fold_bop(rec, ds.objlist, ds.diameter, rr.W)
    assert res["AR_VSD"] == res["AR_MSSD"] == res["AR_MSPD"] == res["AR"] == 1.0 and res["count"] == 3
    with pytest.raises(ValueError, match="meshes"):
        _dataset(root).batch([0], dev, bop=True)


def test_eval_epoch_bop(dev, tree):
    """test_epoch(bop=True) adds the one key "bop"; every other key equals the bop=False run's bit for bit (the
    host and device RNG streams reset to the same state before each run)."""
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd import pose as kpose
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    from pose_estimation_amd.synthetic import init_weights
    root, _ = tree
    m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
    init_weights(m, 0)
    m = m.to(dev).eval()

    def run(**kw):
        torch.manual_seed(5)
        kpose._seeds.clear()
        return run_epoch(m, _dataset(root, **kw), bs=2, device=dev)

    plain = run()
    assert "bop" not in plain
    for opt in ({}, {"opt_pose": False}):
        torch.manual_seed(5)
        kpose._seeds.clear()
        out = run_epoch(m, _dataset(root, meshes=True), bs=2, device=dev, bop=True, **opt)
        res = out.pop("bop")
        print(opt, {k: res[k] for k in sorted(AR_KEYS)})
        assert set(res) == AR_KEYS | {"per_obj"} and set(res["per_obj"]) == {6} and set(res["per_obj"][6]) == AR_KEYS
        assert res["count"] == out["test_count"] == 3
        for k in AR_KEYS - {"count"}:
            assert 0.0 <= res[k] <= 1.0 and res[k] == res["per_obj"][6][k]
        assert abs(res["AR"] - (res["AR_VSD"] + res["AR_MSSD"] + res["AR_MSPD"]) / 3) < 1e-15
        if not opt:
            assert out == plain                                  # every other key, bit for bit
    with pytest.raises(ValueError, match="meshes"):
        run_epoch(m, _dataset(root), bs=2, device=dev, bop=True)
