"""krrn_surface_sample_f64 against its numpy restatement (tests/surface_ref.py), bit for bit, at the tile edges of the
cumulative weights and of the sample grid and on degenerate inputs; an object alone and inside a mixed batch;
oversampling against numpy FPS on the restatement's candidates; bop_scene.write_models_eval's round trip; and
PoseDataset(model_points="surface") on trees whose mesh has fewer vertices than n_model_pts."""
import os

import numpy as np
import pytest
import torch

import bop_scene_ref as sr
import bop_tree
import surface_ref as sf
from oracle.fps_oracle import farthest_point_sampling as fps_ref
from pose_estimation_amd import _lib, bop_scene, models
from pose_estimation_amd.dataset import PoseDataset, ply_faces, ply_vtx
from pose_estimation_amd.runtime import ptr, stream_ptr

pytestmark = pytest.mark.gpu

T = models.SURFACE_TILE
FACES = (1, T - 1, T, T + 1, 3 * T + 17)
SAMPLES = (1, T - 1, T, T + 1)
SEED, STREAM = 11, 2


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _raw(dev, verts, faces, ranges, rows, n, max_f, seed=SEED, stream=STREAM):
    """The entry point itself on a zeroed cum buffer: every output as numpy."""
    v = torch.from_numpy(np.asarray(verts, np.float32)).to(dev)
    f = torch.from_numpy(np.asarray(faces, np.int32).reshape(-1, 3)).to(dev)
    fr = torch.from_numpy(np.asarray(ranges, np.int32).reshape(-1, 2)).to(dev)
    ri = torch.from_numpy(np.asarray(rows, np.int32)).to(dev)
    O = fr.shape[0]
    cum = torch.zeros((O, max_f), dtype=torch.float64, device=dev)
    pts = torch.full((O, n, 3), 9.0, dtype=torch.float32, device=dev)
    nrm = torch.full((O, n, 3), 9.0, dtype=torch.float32, device=dev)
    face = torch.full((O, n), 9, dtype=torch.int32, device=dev)
    status = torch.full((O,), 9, dtype=torch.int32, device=dev)
    _lib.call("krrn_surface_sample_f64", ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(fr), ptr(ri), O, max_f, n, seed,
              stream, ptr(cum), ptr(pts), ptr(nrm), ptr(face), ptr(status), stream_ptr(dev))
    return {"cum": cum.cpu().numpy(), "points": pts.cpu().numpy(), "normals": nrm.cpu().numpy(),
            "face": face.cpu().numpy(), "status": status.cpu().numpy()}


@pytest.fixture(scope="module")
def mixed():
    """Objects of every face count of FACES on random vertices, one with broken faces among good ones, one made only
    of broken faces, and an empty, a negative and a past-the-end range: (names, verts, faces, ranges, rows)."""
    rng = np.random.default_rng(4)
    verts = rng.normal(size=(300, 3)).astype(np.float32)
    verts[299] = [np.nan, 0.5, 0.5]                                        # only the broken faces name it
    objs = {f"f{F}": rng.integers(0, 299, size=(F, 3)) for F in FACES}
    broken = np.array([[299, 1, 2], [5, 5, 9], [3, 4, 300], [-1, 4, 6]])   # NaN corner, zero area, past, negative
    mix = rng.integers(0, 299, size=(40, 3))
    mix[[0, 7, 20, 39]] = broken
    objs["mix"], objs["broken"] = mix, broken
    names, ranges, first = list(objs), [], 0
    for k in names:
        ranges.append((first, len(objs[k])))
        first += len(objs[k])
    faces = np.concatenate([objs[k] for k in names]).astype(np.int32)
    names += ["empty", "negative_first", "negative_count", "past_end"]
    ranges += [(7, 0), (-1, 5), (3, -2), (len(faces) - 2, 5)]
    rows = [3 + 2 * i for i in range(len(names))]
    return names, verts, faces, np.array(ranges, np.int32), rows


@pytest.mark.parametrize("n", SAMPLES)
def test_equals_the_restatement_bit_for_bit(dev, mixed, n):
    names, verts, faces, ranges, rows = mixed
    max_f = max(FACES)
    got = _raw(dev, verts, faces, ranges, rows, n, max_f)
    ref = sf.sample(verts, faces, ranges, rows, n, SEED, STREAM, max_f)
    for key in ("cum", "points", "normals", "face", "status"):
        diff = np.nonzero(_bits(got[key]) != _bits(ref[key].astype(got[key].dtype)))
        assert _same(got[key], ref[key].astype(got[key].dtype)), (key, [d[:4] for d in diff])
    idx = {k: i for i, k in enumerate(names)}
    assert ref["status"].tolist() == [0] * 6 + [1] * 5
    for k in ("broken", "empty", "negative_first", "negative_count", "past_end"):
        o = idx[k]
        assert got["status"][o] == 1 and not got["points"][o].any() and not got["normals"][o].any()
        assert (got["face"][o] == -1).all() and not got["cum"][o].any()
    mix = got["face"][idx["mix"]]
    w, _ = sf.face_weights(verts, faces[ranges[idx["mix"]][0]:][:40])
    assert [k for k in range(40) if w[k] == 0.0] == [0, 7, 20, 39] and not np.isin(mix, [0, 7, 20, 39]).any()
    for F in FACES:                                                        # unit normals, points that are finite
        o = idx[f"f{F}"]
        assert np.isfinite(got["points"][o]).all()
        assert np.allclose(np.linalg.norm(got["normals"][o].astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert (np.diff(got["cum"][o, :F]) >= 0).all() and got["cum"][o, F - 1] > 0


def test_an_object_alone_equals_its_rows_in_the_batch(dev, mixed):
    names, verts, faces, ranges, rows = mixed
    n, max_f = T + 1, max(FACES)
    pick = [names.index(k) for k in ("f1", f"f{T + 1}", "mix", f"f{3 * T + 17}", "broken")]
    batch = _raw(dev, verts, faces, ranges[pick], [rows[o] for o in pick], n, max_f)
    for j, o in enumerate(pick):
        alone = _raw(dev, verts, faces, ranges[o:o + 1], [rows[o]], n, max_f)
        for key in ("cum", "points", "normals", "face", "status"):
            assert _same(alone[key][0], batch[key][j]), (names[o], key)
    o = names.index(f"f{T + 1}")
    base = _raw(dev, verts, faces, ranges[o:o + 1], [rows[o]], n, max_f)
    for kw in (dict(rows=[rows[o] + 1]), dict(rows=[rows[o]], seed=SEED + 1), dict(rows=[rows[o]], stream=STREAM + 1)):
        other = _raw(dev, verts, faces, ranges[o:o + 1], n=n, max_f=max_f, **kw)
        assert _same(other["cum"], base["cum"]) and not np.array_equal(other["points"], base["points"]), kw
    # the same two ranges under the rows swapped: the samples follow the row, not the place in the call
    a = names.index(f"f{T}")
    two = _raw(dev, verts, faces, ranges[[a, a]], [5, 6], n, max_f)
    swapped = _raw(dev, verts, faces, ranges[[a, a]], [6, 5], n, max_f)
    assert _same(two["points"][0], swapped["points"][1]) and _same(two["points"][1], swapped["points"][0])
    assert not np.array_equal(two["points"][0], two["points"][1])


def test_wrapper_and_oversampling_equal_numpy_fps_on_the_restated_candidates(dev, mixed):
    names, verts, faces, ranges, rows = mixed
    pick = [names.index(k) for k in (f"f{T + 1}", "broken", "mix")]          # an object without area between two others
    n, k = 64, 4
    v, f = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    plain = models.sample_surface(v, f, torch.from_numpy(ranges[pick]), n * k, seed=SEED, stream=STREAM,
                                  row_id=[rows[o] for o in pick])
    got = models.sample_surface(v, f, torch.from_numpy(ranges[pick]), n, seed=SEED, stream=STREAM,
                                row_id=[rows[o] for o in pick], oversample=k)
    assert set(got) == {"points", "normals", "face", "status", "area"}
    assert got["points"].shape == (3, n, 3) and got["face"].dtype == torch.int32 and got["area"].dtype == torch.float64
    ref = sf.sample(verts, faces, ranges[pick], [rows[o] for o in pick], n * k, SEED, STREAM, max(FACES))
    assert got["status"].tolist() == [0, 1, 0] and _same(got["area"].cpu().numpy(), ref["area"])
    for key in ("points", "normals", "face"):
        assert _same(plain[key].cpu().numpy(), ref[key]), key               # oversample = 1: the candidates themselves
    for j in range(3):
        if ref["status"][j]:
            assert not got["points"][j].any() and not got["normals"][j].any() and (got["face"][j] == -1).all()
            continue
        keep = fps_ref(ref["points"][j], n)
        assert keep[0] == 0 and len(set(keep.tolist())) == n
        for key in ("points", "normals", "face"):
            assert _same(got[key][j].cpu().numpy(), ref[key][j][keep]), (j, key)
    default_rows = models.sample_surface(v, f, torch.from_numpy(ranges[pick]), 8, seed=SEED, stream=STREAM)
    assert _same(default_rows["points"].cpu().numpy(),
                 sf.sample(verts, faces, ranges[pick], [0, 1, 2], 8, SEED, STREAM, max(FACES))["points"])


def _read_eval(path):
    lines = open(path).read().split("\n")
    head = lines[:lines.index("end_header") + 1]
    body = [ln.split() for ln in lines[len(head):] if ln]
    return head, np.array(body, dtype=np.float64).astype(np.float32)


def test_write_models_eval_round_trip(dev, tmp_path):
    root, one = str(tmp_path / "all"), str(tmp_path / "one")
    bop_tree.write_models(root)
    bop_tree.write_models(one)
    n, k, seed = 96, 4, 3
    paths = bop_scene.write_models_eval(root, dev, n=n, oversample=k, seed=seed)
    objs = sorted(sr.meshes())
    assert sorted(paths) == objs and all(os.path.exists(p) for p in paths.values())
    for obj in objs:
        src = os.path.join(root, "models", f"obj_{obj:06d}.ply")
        mm, tri = ply_vtx(src), ply_faces(src)                              # the file's own unit
        want = models.sample_surface(torch.from_numpy(mm).to(dev), torch.from_numpy(tri).to(dev),
                                     torch.tensor([[0, len(tri)]]), n, seed=seed, row_id=[obj], oversample=k)
        ref = sf.sample_one(mm, tri, n * k, seed, 0, obj)
        keep = fps_ref(ref["points"], n)
        assert _same(want["points"][0].cpu().numpy(), ref["points"][keep])
        assert _same(ply_vtx(paths[obj]), ref["points"][keep]), obj         # the project's own reader: the same f32 bits
        head, rows = _read_eval(paths[obj])
        assert head[:2] == ["ply", "format ascii 1.0"] and head[3] == f"element vertex {n}" and "element face 0" in head
        assert [h.split()[-1] for h in head if h.startswith("property float")] == ["x", "y", "z", "nx", "ny", "nz"]
        assert _same(rows[:, :3], ref["points"][keep]) and _same(rows[:, 3:], ref["normals"][keep])
        assert len(ply_faces(paths[obj])) == 0
        # the points lie on the model: within the box of its vertices, and their count is n
        assert (rows[:, :3] >= mm.min(0)).all() and (rows[:, :3] <= mm.max(0)).all() and rows.shape == (n, 6)
    alone = bop_scene.write_models_eval(one, dev, n=n, oversample=k, seed=seed, objs=[3])
    assert list(alone) == [3] and os.listdir(os.path.join(one, "models_eval")) == ["obj_000003.ply"]
    assert open(alone[3]).read() == open(paths[3]).read()
    with pytest.raises(FileExistsError):
        bop_scene.write_models_eval(root, dev, n=n, oversample=k, seed=seed)
    before = open(paths[2]).read()
    bop_scene.write_models_eval(root, dev, n=n, oversample=k, seed=seed + 1, overwrite=True)
    assert open(paths[2]).read() != before


@pytest.mark.parametrize("layout", ["linemod", "bop"])
def test_dataset_serves_surface_points_where_the_vertices_are_too_few(dev, tmp_path, layout):
    lm, bp = str(tmp_path / "lm"), str(tmp_path / "bop")
    w = bop_tree.write_twin(lm, bp, obj=6, frames=2)
    verts, tri = w["mesh"][6]
    P, seed, k = 300, 5, 4
    assert len(verts) < P
    kw = dict(cls_type="cat", n_model_pts=P, seed=seed, layout=layout, meshes=True)
    root = lm if layout == "linemod" else bp
    with pytest.raises(ValueError, match="num_pt_mesh_large"):
        PoseDataset("test", 100, False, root, 0.0, 8, **kw)                 # the default mode still refuses
    ds = PoseDataset("test", 100, False, root, 0.0, 8, model_points="surface", surface_oversample=k, **kw)
    assert not ds.tree.model_points                                         # nothing sampled before a device is known
    idx = [0, 1] if ds.crop_size(0) == ds.crop_size(1) else [0]
    data = ds.batch(idx, dev)
    want = models.sample_surface(torch.from_numpy(verts).to(dev), torch.from_numpy(tri).to(dev),
                                 torch.tensor([[0, len(tri)]]), P, seed=seed, row_id=[6], oversample=k)
    assert int(want["status"][0]) == 0
    mp = data["model_points"].cpu()
    assert mp.shape == (len(idx), P, 3) and mp.dtype == torch.float32
    for b in range(len(idx)):
        assert _same(mp[b].numpy(), want["points"][0].cpu().numpy())
    assert _same(ds.tree.model_points[6], want["points"][0].cpu().numpy())
    ref = sf.sample_one(verts, tri, P * k, seed, 0, 6)
    assert _same(mp[0].numpy(), ref["points"][fps_ref(ref["points"], P)])
    metas = [ds._meta(i) for i in idx]
    R64 = torch.from_numpy(np.stack([m[1] for m in metas]))
    t64 = torch.from_numpy(np.stack([m[2] for m in metas]))
    target = (mp.double() @ R64.transpose(1, 2) + t64[:, None]).float()     # as the default path forms it
    assert _same(data["target"].cpu().numpy(), target.numpy())
    r = np.linalg.norm(mp[0].numpy().astype(np.float64), axis=1)            # on the icosphere: between its in- and circumradius
    radius = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert r.max() <= radius.max() * (1 + 1e-6) and r.min() >= 0.9 * radius.min()
    again = ds.batch(idx, dev)                                              # cached: the same points on a second batch
    assert _same(again["model_points"].cpu().numpy(), mp.numpy())
