"""numpy restatement of krrn_surface_sample_f64 (include/krrn_hip.h), operation for operation in f64: numpy rounds
every product and sum on its own, as the kernels do without FMA contraction, and np.cumsum adds in index order, so the
two agree bit for bit. Draws come from draws_ref.rand32. Nothing here imports the package.

    w, N = face_weights(verts, faces)                 # f64 [F], f64 [F, 3]
    cum = cumulative(w)                               # f64 [F], tiles of TILE faces
    s = sample_one(verts, faces, n, seed, stream, row)  # {"cum", "points", "normals", "face", "status", "area"}
    s = sample(verts, faces, face_range, row_id, n, seed, stream, max_f)   # the call's outputs, stacked over the objects
"""
import numpy as np

from draws_ref import rand32

TILE = 256  # kSurfTile: the faces per tile of the cumulative sum


def face_weights(verts, faces):
    """(w f64 [F], N f64 [F, 3]) of the faces (indices into verts, the whole array): N = e1 x e2 of the corners widened
    to f64, w = sqrt((Nx Nx + Ny Ny) + Nz Nz) where that is > 0 and finite, else 0; a face with an index outside
    [0, V) has w = 0 (and N = 0 here)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    g = np.where(ok[:, None], f, 0)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        A2 = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        live = ok & (A2 > 0.0) & (A2 < np.inf)
        w = np.where(live, np.sqrt(np.where(live, A2, 1.0)), 0.0)
    return w, np.where(ok[:, None], N, 0.0)


def cumulative(w):
    """cum[k] = base_j + run: within tile j of TILE faces run = run + w_k from 0 in face order; base_0 = 0 and
    base_{j+1} = base_j + the tile's last run."""
    w = np.asarray(w, np.float64)
    cum = np.zeros(len(w), np.float64)
    base = np.float64(0.0)
    for k0 in range(0, len(w), TILE):
        run = np.cumsum(w[k0:k0 + TILE])     # sequential: ((0 + w0) + w1) + ..., and 0 + w0 is w0
        cum[k0:k0 + TILE] = base + run
        base = base + run[-1]
    return cum


def sample_one(verts, faces, n, seed, stream, row):
    """One object's outputs: `faces` are the object's own (its range cut out, indices into the whole `verts`)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    w, N = face_weights(verts, faces)
    cum = cumulative(w)
    total = cum[-1] if F else np.float64(0.0)
    out = {"cum": cum, "points": np.zeros((n, 3), np.float32), "normals": np.zeros((n, 3), np.float32),
           "face": np.full(n, -1, np.int32), "status": 1, "area": float(total) / 2}
    if total == 0.0:
        return out
    i = np.arange(n, dtype=np.uint64)
    r = [rand32(seed, stream, row, np.uint64(4) * i + np.uint64(q)).astype(np.uint64) for q in range(4)]
    m = ((r[0] << np.uint64(32)) | r[1]) >> np.uint64(11)
    target = (m.astype(np.float64) * 2.0 ** -53) * total
    k = np.searchsorted(cum, target, side="right")            # the first k with cum[k] > target
    k = np.where(k < F, k, F - 1)
    v = verts.astype(np.float64)
    fk = faces[k]
    inside = ((fk >= 0) & (fk < len(v))).all(1)               # false only through `none` (a total that is not finite)
    fk = np.where(inside[:, None], fk, 0)
    a, b, c = v[fk[:, 0]], v[fk[:, 1]], v[fk[:, 2]]
    u1, u2 = r[2].astype(np.float64) * 2.0 ** -32, r[3].astype(np.float64) * 2.0 ** -32
    s = np.sqrt(u1)
    wa, wb, wc = 1.0 - s, s * (1.0 - u2), s * u2
    with np.errstate(all="ignore"):
        p = (wa[:, None] * a + wb[:, None] * b) + wc[:, None] * c
        q = N[k] / w[k][:, None]
    out["points"] = np.where(inside[:, None], p, 0.0).astype(np.float32)
    out["normals"] = np.where(inside[:, None], q, 0.0).astype(np.float32)
    out["face"] = k.astype(np.int32)
    out["status"] = 0
    return out


def guarded(rng, Ftot, max_f):
    """(first, count) as the kernels take a face range: negative, longer than max_f or reaching past Ftot is empty."""
    first, count = int(rng[0]), int(rng[1])
    ok = first >= 0 and count >= 0 and count <= max_f and first + count <= Ftot
    return first, (count if ok else 0)


def sample(verts, faces, face_range, row_id, n, seed, stream, max_f):
    """The call's outputs for O objects: {"cum" f64 [O, max_f] (zeros past an object's faces: what a zeroed buffer
    keeps), "points", "normals" f32 [O, n, 3], "face" i32 [O, n], "status" i32 [O], "area" f64 [O]}."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    face_range = np.asarray(face_range).reshape(-1, 2)
    O = len(face_range)
    out = {"cum": np.zeros((O, max_f)), "points": np.zeros((O, n, 3), np.float32),
           "normals": np.zeros((O, n, 3), np.float32), "face": np.zeros((O, n), np.int32),
           "status": np.zeros(O, np.int32), "area": np.zeros(O)}
    for o in range(O):
        f0, nf = guarded(face_range[o], len(faces), max_f)
        one = sample_one(verts, faces[f0:f0 + nf], n, seed, stream, int(row_id[o]))
        out["cum"][o, :nf] = one["cum"]
        for key in ("points", "normals", "face", "status", "area"):
            out[key][o] = one[key]
    return out
