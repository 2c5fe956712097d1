"""The BOP-19 pose errors without a GPU: the numpy restatement (tests/bop_ref.py) on its scene family (decision
margins, known answers, a ray-cast cross-check of its depth images), bop.symmetry_set, bop.fold_bop against a
per-crop loop, evaluate.gather_epoch_records at the BOP table's width over gloo world-2, the host-side argument
checks of krrn_bop_vsd_f32 / krrn_bop_mssd_mspd_f32 (they run before any HIP call) and the dataset's errors."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bop_ref as br
import raster_ref as rr
from pose_estimation_amd import _lib, bop
from pose_estimation_amd.dataset import PoseDataset


# ------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("name", br.SCENES)
def test_scene_conditions(name):
    """Zero undecided pixels in every scene: no pixel is left out of the GPU comparison."""
    res = br.reference(name)
    print(name, res["counts"].tolist(), {k: float(v.min()) for k, v in res["margins"].items()})
    br.check_conditions(res)
    assert res["counts"][0] > 0
    assert (np.diff(res["e_vsd"]) <= 0).all()                   # non-increasing in tau
    assert (np.diff(res["counts"][2:]) <= 0).all()


def test_mixed_conditions():
    bt, crops, frames = br.mixed()
    assert frames.shape == (rr.MIXED_B, rr.H, rr.W) and frames.dtype == np.float32
    for b in range(rr.MIXED_B):
        res = br.mixed_reference(b)
        br.check_conditions(res)
        assert (res["counts"][0] > 0) == (b != 3)
    empty = br.mixed_reference(3)                                # the crop with an empty face range
    assert not empty["counts"].any() and (empty["e_vsd"] == 1.0).all()


@pytest.mark.parametrize("name", ["tetra", "sphere", "small"])
def test_estimate_equal_to_gt(name):
    sc = br.scene(name)
    res = br.scene_vsd(sc, R_est=sc["R_gt"], t_est=sc["t_gt"])
    assert (res["e_vsd"] == 0.0).all() and not res["counts"][2:].any()
    assert res["counts"][0] == res["counts"][1] == int(res["v_gt"].sum()) > 0
    # some of the GT silhouette is occluded or ... not: pixels of a hole are visible by the obs == 0 rule
    assert int(res["v_gt"].sum()) < int((res["d_gt"] > 0).sum())
    mssd, mspd, i3, i2, _, _ = br.mssd_mspd(sc["verts"], sc["R_gt"], sc["t_gt"], sc["R_gt"], sc["t_gt"], sc["K4"],
                                            bop.symmetry_set())
    assert mssd == 0.0 and mspd == 0.0 and i3 == i2 == 0


def test_gross_estimate_and_empty_observation():
    res = br.reference("gross")                                  # wholly off the GT silhouette
    assert not ((res["d_est"] > 0) & (res["d_gt"] > 0)).any()
    assert res["counts"][1] == 0 and res["counts"][0] > 0 and (res["e_vsd"] == 1.0).all()
    res = br.reference("empty_obs")                              # obs == 0 everywhere: both renders wholly visible
    assert res["counts"][0] == int(((res["d_est"] > 0) | (res["d_gt"] > 0)).sum())
    assert res["counts"][1] == int(((res["d_est"] > 0) & (res["d_gt"] > 0)).sum())


@pytest.mark.parametrize("name", br.RAYCAST)
def test_depth_images_against_ray_casting(name):
    """The same counts from depth images made by 3-D ray / triangle intersection, which shares no code with the
    rasteriser's 2-D edge functions."""
    sc, ref = br.scene(name), br.reference(name)
    S = max(sc["H"], sc["W"])
    imgs = []
    for R, t in ((sc["R_est"], sc["t_est"]), (sc["R_gt"], sc["t_gt"])):
        _, d = rr.raycast(sc["verts"], sc["faces"], R, t, sc["K4"], 0, 0, S)
        imgs.append(d[:sc["H"], :sc["W"]])
    assert np.abs(imgs[0] - ref["d_est"]).max() < 1e-12 and np.abs(imgs[1] - ref["d_gt"]).max() < 1e-12
    res = br.scene_vsd(sc, images=tuple(imgs))
    assert np.array_equal(res["counts"], ref["counts"])
    assert np.array_equal(res["e_vsd"], ref["e_vsd"])


def test_symmetric_tetrahedron():
    """est = GT o S for the 180-degree symmetry S: MSSD is 0 to rounding with the set, > 0 with the identity only."""
    v, S = br.sym_tetra()
    rng = np.random.default_rng(3)
    R_gt, t_gt = rr.rotation(rng), rr._centre_t(0.7, 300.2, 220.6)
    Rs, ts = S[1, :9].reshape(3, 3), S[1, 9:]
    R_est, t_est = R_gt @ Rs, R_gt @ ts + t_gt
    with_set = br.mssd_mspd(v, R_est, t_est, R_gt, t_gt, rr.LM_K4, S)
    alone = br.mssd_mspd(v, R_est, t_est, R_gt, t_gt, rr.LM_K4, S[:1])
    print(with_set[:4], alone[:4])
    assert with_set[0] < 1e-14 and with_set[1] < 1e-10 and with_set[2] == with_set[3] == 1
    assert alone[0] > 0.02 and alone[1] > 10.0
    assert br.mssd_mspd(v[:0], R_est, t_est, R_gt, t_gt, rr.LM_K4, S)[:4] == (np.inf, np.inf, -1, -1)
    assert br.mssd_mspd(v, R_est, t_est, R_gt, t_gt, rr.LM_K4, S[:0])[:4] == (np.inf, np.inf, -1, -1)


# ------------------------------------------------------------------------------------------ symmetry_set

def _orthonormal(S):
    R = S[:, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-12


def test_symmetry_set():
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    S = bop.symmetry_set()
    assert S.shape == (1, 12) and S.dtype == np.float64 and np.array_equal(S[0], ident)
    flip = [-1, 0, 0, 10.0, 0, -1, 0, -4.0, 0, 0, 1, 0, 0, 0, 0, 1]             # translation in mm
    S = bop.symmetry_set(discrete=[flip], diameter_m=0.1)
    assert S.shape == (2, 12) and np.array_equal(S[0], ident)
    assert np.array_equal(S[1], [-1, 0, 0, 0, -1, 0, 0, 0, 1, 0.01, -0.004, 0])  # mm -> m
    assert bop.symmetry_set(discrete=[flip, flip, np.eye(4)]).shape == (2, 12)   # de-duplicated
    n = int(math.ceil(math.pi / 0.01))
    assert n == 315
    S = bop.symmetry_set(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}])
    assert S.shape == (n, 12) and np.array_equal(S[0], ident)
    _orthonormal(S)
    ang = np.arctan2(S[:, 3], S[:, 0]) % (2 * np.pi)
    assert np.abs(np.sort(ang) - 2 * np.pi * np.arange(n) / n).max() < 1e-12     # equal steps about the axis
    assert not S[:, 9:].any()
    off = bop.symmetry_set(continuous=[{"axis": [0, 1, 0], "offset": [20.0, 0, 0]}], max_step=0.5)
    assert off.shape == (7, 12)
    _orthonormal(off)
    for row in off:                                              # a point on the axis stays put
        assert np.abs(row[:9].reshape(3, 3) @ [0.02, 0.3, 0.0] + row[9:] - [0.02, 0.3, 0.0]).max() < 1e-15
    both = bop.symmetry_set(discrete=[[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]],
                            continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}], max_step=0.5)
    assert both.shape == (14, 12)                                # every combination
    _orthonormal(both)


# ------------------------------------------------------------------------------------------ fold_bop

def _loop(rec, objlist, diameter, width):
    rec = rec[rec[:, -1] > 0]
    rec = rec[np.argsort(rec[:, 0], kind="stable")]
    T = len(bop.TAUS)

    def fold(rows):
        if not len(rows):
            return {"AR_VSD": 0.0, "AR_MSSD": 0.0, "AR_MSPD": 0.0, "AR": 0.0, "count": 0}
        v = m = p = 0
        for row in rows:
            dia = diameter[int(row[1])]
            for k in range(1, 11):
                v += sum(1 for e in row[2:2 + T] if e < 0.05 * k)
                m += row[2 + T] < 0.05 * k * dia
                p += row[3 + T] < 5.0 * k * (width / 640.0)
        n = len(rows)
        a = (v / (n * T * 10), m / (n * 10), p / (n * 10))
        return {"AR_VSD": a[0], "AR_MSSD": a[1], "AR_MSPD": a[2], "AR": sum(a) / 3, "count": n}

    out = fold(rec)
    out["per_obj"] = {objlist[c]: fold(rec[rec[:, 1] == c]) for c in dict.fromkeys(rec[:, 1].astype(int).tolist())}
    return out


@pytest.mark.parametrize("n,ncls,width", [(500, 13, 640), (37, 5, 320), (1, 13, 640), (0, 13, 640)])
def test_fold_bop_against_loop(n, ncls, width):
    from pose_estimation_amd.config import LM_OBJLIST
    rng = np.random.default_rng(n)
    objlist, diameter = LM_OBJLIST[:ncls], [0.1 + 0.01 * i for i in range(ncls)]
    T = len(bop.TAUS)
    assert len(bop.BOP_REC) == T + 5 and bop.BOP_REC[0] == "crop" and bop.BOP_REC[-1] == "valid"
    rec = np.zeros((n + 3, len(bop.BOP_REC)))
    rec[:n, 0] = rng.permutation(n)
    rec[:n, 1] = rng.integers(0, ncls, n)
    rec[:n, 2:2 + T] = np.sort(rng.random((n, T)) * 0.8, 1)[:, ::-1]
    rec[:n, 2 + T] = rng.random(n) * 0.08
    rec[:n, 3 + T] = rng.random(n) * 60 * width / 640
    rec[:n, -1] = 1.0
    if n > 4:                                                    # exact ties: strict <
        rec[0, 2] = 0.05 * 3
        rec[1, 2 + T] = 0.05 * 2 * diameter[int(rec[1, 1])]
        rec[2, 3 + T] = 5.0 * 4 * (width / 640.0)
    got = bop.fold_bop(torch.from_numpy(rec), objlist, diameter, width)
    exp = _loop(rec, objlist, diameter, width)
    assert set(got) == {"AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "count", "per_obj"}
    assert got["count"] == exp["count"] == n and list(got["per_obj"]) == list(exp["per_obj"])
    for a, b in [(got, exp)] + [(got["per_obj"][o], exp["per_obj"][o]) for o in exp["per_obj"]]:
        assert a["count"] == b["count"]
        for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
            assert abs(a[k] - b[k]) < 1e-12, (k, a[k], b[k])
    assert bop.fold_bop(rec[rng.permutation(len(rec))], objlist, diameter, width) == got   # any row order
    perfect = rec.copy()
    perfect[:, 2:4 + T] = 0.0
    if n:
        assert bop.fold_bop(perfect, objlist, diameter, width)["AR"] == 1.0


# ------------------------------------------------------------------------------------------ gather

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _table(rank, rows, width):
    t = torch.arange(rows * width, dtype=torch.float64).reshape(rows, width) + 1000.0 * rank
    t[:, -1] = 1.0
    return t


def _gather_worker(rank, world, port, shard_sizes, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from pose_estimation_amd import distributed as kd
    from pose_estimation_amd import evaluate as ev
    kd.init_from_env("gloo")
    out = {}
    for width in (len(ev.REC), len(bop.BOP_REC)):
        out[width] = ev.gather_epoch_records(_table(rank, shard_sizes[rank], width), shard_sizes, "cpu").tolist()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_gather_at_both_widths():
    from pose_estimation_amd import evaluate as ev
    assert len(bop.BOP_REC) != len(ev.REC)
    shard_sizes = [5, 3]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, shard_sizes, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, out in res:
        for width in (len(ev.REC), len(bop.BOP_REC)):
            t = torch.tensor(out[width], dtype=torch.float64)
            assert t.shape == (2 * max(shard_sizes), width)
            for r in range(2):
                blk = t[5 * r:5 * (r + 1)]
                assert torch.equal(blk[:shard_sizes[r]], _table(r, shard_sizes[r], width))
                assert not blk[shard_sizes[r]:].any()            # pad rows: valid = 0


# ------------------------------------------------------------------------------------------ host checks

def _fakes(names):
    """Distinct, far-apart non-null pointers (never dereferenced: the checks fail before any launch)."""
    return {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(names)}


def test_vsd_host_side_errors():
    fn = _lib.lib().krrn_bop_vsd_f32
    N, D = ctypes.c_void_p(0), ctypes.c_double
    names = ("verts", "faces", "face_range", "R_est", "t_est", "R_gt", "t_gt", "K4", "depth", "frame", "diameter",
             "taus", "ws", "counts", "e_vsd")

    def call(V=10, Ft=4, F=2, H=480, W=640, scale=1000.0, delta=0.015, T=10, B=2, **over):
        p = _fakes(names)
        p.update(over)
        return fn(p["verts"], V, p["faces"], Ft, p["face_range"], p["R_est"], p["t_est"], p["R_gt"], p["t_gt"], p["K4"],
                  p["depth"], F, H, W, p["frame"], D(scale), p["diameter"], D(delta), p["taus"], T, B, p["ws"],
                  p["counts"], p["e_vsd"], N)

    for k in names:
        assert call(**{k: N}) == -1, k
    f = _fakes(names)
    assert call(counts=f["e_vsd"]) == -1                         # two outputs on one buffer
    assert call(e_vsd=f["R_gt"]) == -1 and call(ws=f["frame"]) == -1   # an output on an input
    assert call(counts=ctypes.c_void_p(f["depth"].value + 4 * 480 * 640)) == -1   # inside the second frame
    assert call(T=0) == -2 and call(T=17) == -2 and call(T=-1) == -2
    assert call(delta=0.0) == -2 and call(delta=-0.015) == -2 and call(delta=float("nan")) == -2
    assert call(scale=0.0) == -2 and call(scale=-1.0) == -2
    assert call(B=0) == -2 and call(V=0) == -2 and call(H=0) == -2 and call(W=0) == -2 and call(F=0) == -2
    assert call(Ft=-1) == -2
    assert call(T=17, taus=N) == -1                              # pointers are checked first
    n = ctypes.c_longlong(0)
    ws = _lib.lib().krrn_bop_vsd_ws
    assert ws(3, ctypes.byref(n)) == 0 and n.value == 24
    assert ws(0, ctypes.byref(n)) == -2 and ws(3, N) == -1


def test_mssd_mspd_host_side_errors():
    fn = _lib.lib().krrn_bop_mssd_mspd_f32
    N = ctypes.c_void_p(0)
    names = ("verts", "vert_range", "R_est", "t_est", "R_gt", "t_gt", "K4", "syms", "sym_range", "ws", "mssd", "mspd",
             "idx")

    def call(V=10, NS=2, B=2, **over):
        p = _fakes(names)
        p.update(over)
        return fn(p["verts"], V, p["vert_range"], p["R_est"], p["t_est"], p["R_gt"], p["t_gt"], p["K4"], p["syms"], NS,
                  p["sym_range"], B, p["ws"], p["mssd"], p["mspd"], p["idx"], N)

    for k in names[:-1]:                                         # sym_idx is optional
        assert call(**{k: N}) == -1, k
    f = _fakes(names)
    assert call(mspd=f["mssd"]) == -1 and call(mssd=f["syms"]) == -1 and call(idx=f["K4"]) == -1
    assert call(mspd=ctypes.c_void_p(f["mssd"].value + 8)) == -1 and call(ws=f["vert_range"]) == -1
    assert call(mssd=ctypes.c_void_p(f["ws"].value + 8 * 3 * 2 * bop.SYM_SPLIT - 8)) == -1   # the last ws double
    n = ctypes.c_longlong(0)
    ws = _lib.lib().krrn_bop_mssd_mspd_ws
    assert ws(2, ctypes.byref(n)) == 0 and n.value == 3 * 2 * bop.SYM_SPLIT
    assert ws(0, ctypes.byref(n)) == -2 and ws(2, N) == -1
    assert call(B=0) == -2 and call(V=0) == -2 and call(NS=0) == -2
    assert call(B=0, verts=N) == -1


def test_abi_lists_the_entry_points():
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.SIGNATURES["krrn_bop_vsd_f32"] == [P, I, P, I] + [P] * 7 + [I, I, I, P, D, P, D, P, I, I, P, P, P, P]
    assert _lib.SIGNATURES["krrn_bop_mssd_mspd_f32"] == [P, I] + [P] * 7 + [I, P, I, P, P, P, P, P]
    assert _lib.SIGNATURES["krrn_bop_vsd_ws"] == [I, P] == _lib.SIGNATURES["krrn_bop_mssd_mspd_ws"]


# ------------------------------------------------------------------------------------------ python layer

def test_cpu_tensors_raise():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP path only"):
        bop.vsd(z(4, 3), z(2, 3, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 3, 3), z(1, 3), z(1, 3, 3), z(1, 3),
                z(1, 4), z(1, 8, 8), z(1, dtype=torch.int32), z(1))
    with pytest.raises(RuntimeError, match="HIP path only"):
        bop.mssd_mspd(z(4, 3), z(1, 2, dtype=torch.int32), z(1, 3, 3), z(1, 3), z(1, 3, 3), z(1, 3), z(1, 4), z(1, 12),
                      z(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="bop=True"):
        bop.bop_errors(z(1, 3, 3), z(1, 3), {"cls_id": z(1, 1)}, None)
    assert len(bop.TAUS) == len(bop.THETAS) == len(bop.THETAS_PX) == 10 and bop.DELTA == 0.015
    assert abs(bop.TAUS[-1] - 0.5) < 1e-15 and bop.THETAS_PX[-1] == 50.0


def test_dataset_meshes_and_symmetries(tmp_path):
    import yaml

    import linemod_tree
    import mesh_tree
    with pytest.raises(ValueError, match="root=None"):
        PoseDataset("test", 500, False, None, 0.0, 8, cls_type="cat", meshes=True)
    plain = PoseDataset("test", 500, False, None, 0.0, 8, cls_type="cat", num_frames=2)
    with pytest.raises(ValueError, match="meshes"):
        plain.batch([0], "cpu", bop=True)
    linemod_tree.write_tree(str(tmp_path / "a"), objs=(6,), per_obj=1, sizes=(80,))
    with pytest.raises(ValueError, match="obj_06.ply has no faces"):
        PoseDataset("test", 500, False, str(tmp_path / "a"), 0.0, 8, cls_type="cat", meshes=True)
    root = str(tmp_path / "b")
    mesh_tree.write_tree(root, objs=(6,), per_obj=(1,))
    ds = PoseDataset("test", 100, False, root, 0.0, 8, cls_type="cat", n_model_pts=100, meshes=True)
    assert ds.meshes and not ds.gt_maps and ds.tree.mesh[6][1].shape == (320, 3)
    assert ds.tree.symmetries[6].shape == (1, 12)                # a stock tree: the identity only
    assert PoseDataset("test", 100, False, root, 0.0, 8, cls_type="cat", n_model_pts=100, gt_maps=True).meshes
    with open(os.path.join(root, "models", "models_info.yml"), "w") as fh:
        yaml.safe_dump({6: {"diameter": 60.0, "symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]},
                        2: {"diameter": 60.0}}, fh)
    ds = PoseDataset("test", 100, False, root, 0.0, 8, cls_type="cat", n_model_pts=100, meshes=True)
    assert ds.tree.symmetries[6].shape == (2, 12)
    assert np.array_equal(ds.tree.symmetries[6][1], [-1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0])
