"""krrn_model_extent_f64 and krrn_symmetry_residual_f64 against their numpy restatement (tests/models_ref.py), bit for
bit, at the kernels' tile edges and degenerate inputs; each object's and symmetry's outputs alone and inside the mixed
batch; and bop_scene.write_models_info / check_models_info on the tiny tree of tests/bop_tree.py."""
import json
import os

import numpy as np
import pytest
import torch

import bop_scene_ref as sr
import bop_tree
import models_ref as mr
from pose_estimation_amd import bop, bop_scene, models
from pose_estimation_amd.dataset import PoseDataset

pytestmark = pytest.mark.gpu

R, C = models.EXTENT_R, models.EXTENT_C
RV, RF = models.RESIDUAL_R, models.RESIDUAL_C
SIZES = (0, 1, 2, R - 1, R, R + 1, 2 * R + 3, C + 1)
V_PLANT = 2 * R + 3
PLANTS = {"in_tile": (5, 100), "tile_edge": (R - 1, R), "first_last": (0, V_PLANT - 1),
          "last_partial": (2 * R + 1, 2 * R + 2)}
EYE = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
Z180 = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]            # bop_tree.write_models' declared symmetry


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _planted(rng, n, i, j):
    v = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    v[i], v[j] = (-7.25, 6.5, -5.125), (7.5, -6.25, 5.75)
    return v


@pytest.fixture(scope="module")
def ext_case(dev):
    """The mixed extent batch: ({name: object index}, verts, ranges, the batch's result, the restatement's)."""
    rng = np.random.default_rng(3)
    objs = {f"v{n}": rng.normal(size=(n, 3)).astype(np.float32) for n in SIZES}
    for name, (i, j) in PLANTS.items():
        objs[name] = _planted(rng, V_PLANT, i, j)
    objs["col_edge"] = _planted(rng, C + 1, C - 1, C)                # across the column tile's edge
    objs["same"] = np.tile(np.float32([0.3, -1.7, 2.9]), (R + 44, 1))
    nan = rng.normal(size=(R + 44, 3)).astype(np.float32)
    nan[17], nan[R + 3, 1] = np.nan, np.nan                         # a NaN vertex, and one NaN coordinate
    nan[R + 3, 0] = 50.0                                            # the largest x by far, beside a NaN y
    objs["nan"] = nan
    corners = np.array([[x, y, z] for x in (0, 3) for y in (0, 4) for z in (0, 12)], np.float32)
    objs["box"] = np.concatenate([corners, rng.integers(1, 3, size=(40, 3)).astype(np.float32)])
    names, ranges, first = list(objs), [], 0
    for k in names:
        ranges.append((first, len(objs[k])))
        first += len(objs[k])
    verts = np.concatenate([objs[k] for k in names])
    names += ["negative_first", "negative_count", "past_end"]
    ranges += [(-1, 5), (3, -2), (len(verts) - 2, 5)]
    ranges = np.array(ranges, np.int32)
    got = models.extent(torch.from_numpy(verts).to(dev), torch.from_numpy(ranges))
    return {k: i for i, k in enumerate(names)}, verts, ranges, got, mr.extent(verts, ranges)


def test_extent_equals_the_restatement_bit_for_bit(ext_case):
    idx, verts, ranges, got, (d2, box) = ext_case
    assert _same(got["d2"], d2)
    assert _same(got["min"], box[:, :3]) and _same(got["max"], box[:, 3:])
    assert _same(got["size"], box[:, 3:] - box[:, :3])
    assert _same(got["diameter"], np.sqrt(d2))
    for n in SIZES[3:]:
        assert d2[idx[f"v{n}"]] > 0.0


def test_extent_finds_the_planted_pair(ext_case):
    idx, verts, ranges, got, _ = ext_case
    want = float(np.sum((np.float64([7.5, -6.25, 5.75]) - np.float64([-7.25, 6.5, -5.125])) ** 2))   # exact in f64
    for name in list(PLANTS) + ["col_edge"]:
        assert float(got["d2"][idx[name]]) == want, name


def test_extent_degenerate_objects(ext_case):
    idx, verts, ranges, got, _ = ext_case
    for name in ("v0", "v1", "same"):
        assert float(got["d2"][idx[name]]) == 0.0, name
    assert float(got["d2"][idx["box"]]) == 169.0                    # 3^2 + 4^2 + 12^2: the constant, not the restatement
    assert got["min"][idx["box"]].tolist() == [0.0, 0.0, 0.0] and got["size"][idx["box"]].tolist() == [3.0, 4.0, 12.0]
    for name in ("v0", "negative_first", "negative_count", "past_end"):
        o = idx[name]
        assert float(got["d2"][o]) == 0.0, name
        assert got["min"][o].tolist() == [np.inf] * 3 and got["max"][o].tolist() == [-np.inf] * 3, name
    o = idx["nan"]
    f0, n = ranges[o]
    clean = np.delete(verts[f0:f0 + n], [17, R + 3], axis=0)
    d2_clean, box_clean = mr.extent_one(clean)
    assert float(got["d2"][o]) == d2_clean                          # the NaN vertices take no part in d2
    assert np.isfinite(got["min"][o].numpy()).all()
    assert float(got["max"][o][0]) == 50.0                          # the finite coordinates of a half-NaN vertex count
    assert got["min"][o].tolist()[1:] == box_clean[1:3].tolist()


def test_extent_does_not_depend_on_the_batch(ext_case, dev):
    idx, verts, ranges, got, _ = ext_case
    v = torch.from_numpy(verts).to(dev)
    for name, o in idx.items():
        alone = models.extent(v, torch.from_numpy(ranges[o:o + 1]))
        for k in ("d2", "min", "max"):
            assert _same(alone[k][0], got[k][o]), (name, k)
    o = idx["tile_edge"]                                            # and with the object's vertices as the whole buffer
    f0, n = ranges[o]
    own = models.extent(torch.from_numpy(verts[f0:f0 + n].copy()).to(dev), torch.tensor([[0, int(n)]]))
    assert _same(own["d2"][0], got["d2"][o]) and _same(own["min"][0], got["min"][o])


def _prism():
    v = np.array([[x, y, z] for z in (-2, 2) for x, y in ((1, 1), (-1, 1), (-1, -1), (1, -1))], np.float32)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6]]
    for k in range(4):
        a, b = k, (k + 1) % 4
        f += [[a, b, b + 4], [a, b + 4, a + 4]]
    return v, np.array(f, np.int32)


def _rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([c, -s, 0, s, c, 0, 0, 0, 1, 0, 0, 0], np.float64)


@pytest.fixture(scope="module")
def res_case(dev):
    """The mixed residual batch: ({name: (object index, first symmetry, count)}, operands, the batch's res2, the
    restatement's)."""
    rng = np.random.default_rng(4)
    objs = []                                                       # (name, verts, faces local, syms [n, 12])
    for obj, (v, f) in sr.meshes().items():
        objs.append((f"mesh{obj}", v, f, bop.symmetry_set(discrete=[Z180])))
    pv, pf = _prism()
    z90 = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0], np.float64)
    objs.append(("prism", pv, pf, np.stack([EYE, z90, _rot_z(45.0)])))
    some = rng.normal(size=(12,)) * 0.5
    for nv, nf in ((3, 1), (RV - 1, RF - 1), (RV + 1, RF), (2 * RV + 3, RF + 1)):
        v = rng.normal(size=(nv, 3)).astype(np.float32)
        f = rng.integers(0, nv, size=(nf, 3)).astype(np.int32)
        if nf > RF:
            v[:3] = (0, 0, 0), (2, 2, 2), (0.5, 0.5, 0.5)
            f[7] = (0, 1, 2)                                        # collinear, three distinct corners
            f[RF] = (5, 5, 5)                                       # collapsed to a point, in the last, partial tile
            f[RF - 1] = (0, 1, 10 ** 6)                             # names a vertex that does not exist: skipped
            f[3] = (-1, 1, 2)
        objs.append((f"f{nf}", v, f, np.stack([EYE, some])))
    tet_v, tet_f = sr.meshes()[1]
    objs.append(("nan_vertex", np.concatenate([tet_v, np.float32([[np.nan, 0, 0]])]), tet_f, EYE[None]))
    objs.append(("no_vertices", np.zeros((0, 3), np.float32), tet_f[:0], EYE[None]))
    names, vs, fs, ss, vr, fr, srg = [], [], [], [], [], [], []
    v0 = f0 = s0 = 0
    for name, v, f, s in objs:
        names.append(name)
        vs.append(v), fs.append(f.astype(np.int64) + _shift(f, v0)), ss.append(s)
        vr.append((v0, len(v))), fr.append((f0, len(f))), srg.append((s0, len(s)))
        v0, f0, s0 = v0 + len(v), f0 + len(f), s0 + len(s)
    names += ["no_faces", "faces_past_end"]                          # the prism's vertices without a usable face range
    prism = names.index("prism")
    vr += [vr[prism], vr[prism]]
    fr += [(3, 0), (f0 - 2, 5)]
    srg += [(s0, 1), (s0 + 1, 1)]
    ss.append(np.stack([EYE, EYE, EYE]))                            # the last row is owned by nobody
    verts, faces, syms = np.concatenate(vs), np.concatenate(fs).astype(np.int32), np.concatenate(ss)
    vr, fr, srg = (np.array(x, np.int32) for x in (vr, fr, srg))
    t = lambda x: torch.from_numpy(x)                               # noqa: E731
    got = models.symmetry_residual(t(verts).to(dev), t(faces).to(dev), t(vr), t(fr), t(syms), t(srg), squared=True)
    ref = mr.residual(verts, faces, vr, fr, syms, srg)
    return ({k: (i, int(srg[i][0]), int(srg[i][1])) for i, k in enumerate(names)}, (verts, faces, vr, fr, syms, srg),
            got.numpy(), ref)


def _shift(f, v0):
    """Local face indices to indices into the concatenated vertices; the two deliberately bad indices stay bad."""
    f = f.astype(np.int64)
    return np.where((f >= 0) & (f < 10 ** 6), v0, 0)


def test_residual_equals_the_restatement_bit_for_bit(res_case):
    idx, _, got, ref = res_case
    assert _same(got, ref)
    assert np.isnan(got[-1]) and not np.isnan(got[:-1]).any()       # the row nobody owns kept the wrapper's fill


def test_residual_of_exact_and_wrong_symmetries(res_case):
    idx, _, got, ref = res_case
    for name in ("mesh1", "mesh2", "mesh3", "prism"):
        assert got[idx[name][1]] == 0.0, name                       # the identity: every vertex is a corner of a face
    _, s0, n = idx["prism"]
    assert n == 3 and got[s0 + 1] == 0.0                            # the exact quarter turn
    assert got[s0 + 2] > 0.0 and np.isfinite(got[s0 + 2])           # 45 degrees moves the corners off the surface
    for name in ("mesh1", "mesh2", "mesh3"):                        # the declared half turn: finite, whatever it is
        _, s0, n = idx[name]
        assert n == 2 and np.isfinite(got[s0 + 1])
    _, s0, _ = idx[f"f{RF + 1}"]
    assert np.isfinite(got[s0 + 1]) and got[s0 + 1] > 0.0           # the degenerate faces did not poison the walk


def test_residual_of_broken_input(res_case):
    idx, _, got, _ = res_case
    for name in ("no_faces", "faces_past_end", "nan_vertex"):
        assert got[idx[name][1]] == np.inf, name
    assert got[idx["no_vertices"][1]] == 0.0


def test_residual_does_not_depend_on_the_batch(res_case, dev):
    idx, (verts, faces, vr, fr, syms, srg), got, _ = res_case
    t = lambda x: torch.from_numpy(x)                               # noqa: E731
    v, f = t(verts).to(dev), t(faces).to(dev)
    for name, (o, s0, n) in idx.items():
        alone = models.symmetry_residual(v, f, t(vr[o:o + 1]), t(fr[o:o + 1]), t(syms), t(srg[o:o + 1]), squared=True).numpy()
        assert _same(alone[s0:s0 + n], got[s0:s0 + n]), name
        assert np.isnan(np.delete(alone, range(s0, s0 + n))).all(), name   # and nothing else was written
        for s in range(s0, s0 + n):                                 # each symmetry on its own
            one = models.symmetry_residual(v, f, t(vr[o:o + 1]), t(fr[o:o + 1]), t(syms[s:s + 1].copy()),
                                           torch.tensor([[0, 1]]), squared=True).numpy()
            assert _same(one, got[s:s + 1]), (name, s)
    root = models.symmetry_residual(v, f, t(vr), t(fr), t(syms), t(srg)).numpy()
    assert _same(root[:-1], np.sqrt(got[:-1]))                      # the default returns the distance itself


def test_write_models_info_on_a_tree(tmp_path, dev):
    root = str(tmp_path)
    bop_tree.write_tree(root, sym_obj=(2,))
    path = os.path.join(root, "models", "models_info.json")
    with open(path) as fh:
        helper = {int(k): v for k, v in json.load(fh).items()}
    os.remove(path)
    with pytest.raises(FileNotFoundError):
        bop_scene.BopTree(root)
    wrote = bop_scene.write_models_info(root, dev)
    with open(path) as fh:
        made = {int(k): v for k, v in json.load(fh).items()}
    assert sorted(made) == sorted(helper) == sorted(wrote) == sorted(bop_scene.model_info(root, dev, objs=[1, 2, 3]))
    for obj, e in helper.items():
        assert set(made[obj]) == set(bop_scene.MODEL_KEYS)          # the symmetries are not produced
        assert abs(made[obj]["diameter"] - e["diameter"]) <= 1e-12 * e["diameter"], obj
        for k in bop_scene.MODEL_KEYS[1:]:
            assert made[obj][k] == e[k], (obj, k)
    ds = PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True)
    assert len(ds) > 0 and ds.diameter == [made[o]["diameter"] / 1000.0 for o in ds.objlist]
    with pytest.raises(FileExistsError):
        bop_scene.write_models_info(root, dev)

    with open(path, "w") as fh:                                     # the helper's file again: object 2 declares Z180
        json.dump({str(k): v for k, v in helper.items()}, fh)
    again = bop_scene.write_models_info(root, dev, overwrite=True)
    with open(path) as fh:
        kept = {int(k): v for k, v in json.load(fh).items()}
    assert kept[2]["symmetries_discrete"] == helper[2]["symmetries_discrete"] == again[2]["symmetries_discrete"]
    assert "symmetries_discrete" not in kept[1] and "symmetries_discrete" not in kept[3]
    assert all(kept[o][k] == made[o][k] for o in made for k in bop_scene.MODEL_KEYS)

    rep = bop_scene.check_models_info(root, dev)
    meshes = sr.meshes()
    for obj in (1, 2, 3):
        v, f = meshes[obj]
        assert rep[obj]["extent_diff"] == 0.0 and rep[obj]["diameter_file"] == kept[obj]["diameter"] == rep[obj]["diameter"]
        sset = bop.symmetry_set(kept[obj].get("symmetries_discrete"))
        dia_m = np.sqrt(mr.extent_one(v)[0]) * 1000.0 / 1000.0
        want = [float(np.sqrt(mr.residual_one(v, f, (0, len(v)), (0, len(f)), s)) / dia_m) for s in sset]
        assert len(sset) == (2 if obj == 2 else 1) and rep[obj]["residual"] == want, obj
        assert rep[obj]["worst"] == int(np.argmax(want)) and rep[obj]["residual"][0] == 0.0
    assert "residual" not in bop_scene.check_models_info(root, dev, syms=False)[2]
