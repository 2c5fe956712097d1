"""Object-model facts on the GPU: what BOP's calc_model_info script computes (the diameter and the axis-aligned box of
every model), and how well a declared symmetry maps a mesh onto itself (include/krrn_hip.h states both definitions,
tests/models_ref.py restates them in numpy).

    e = extent(verts, vert_range)
    # -> {"d2": f64 [O], "diameter": f64 [O] = sqrt(d2), "min", "max": f64 [O, 3], "size": f64 [O, 3] = max - min}, host values
    r = symmetry_residual(verts, faces, vert_range, face_range, syms, sym_range)
    # -> f64 [NStot], host values: per symmetry the largest distance from a transformed vertex to the surface

    s = sample_surface(verts, faces, face_range, n, seed=0, oversample=4)
    # -> {"points", "normals": f32 [O, n, 3], "face": i32 [O, n], "status": i32 [O], "area": f64 [O]}, GPU tensors: n
    #    points per object drawn uniformly on its surface (krrn_surface_sample_f64), thinned by FPS with oversample > 1

The first two are in the vertices' own unit (the symmetries' translations too). The diameter is the maximum over all vertex
pairs, O(V^2): an all-pairs walk that a [V, V, 3] numpy broadcast cannot hold beyond toy meshes. The residual reports
and does not judge: 0 for an exact symmetry of the mesh, about the tessellation's sag for a symmetry of the shape the
mesh approximates, and a sizeable part of the diameter for a wrong entry (an mm / m mix-up, a wrong axis, an offset
that is not on the axis). bop_scene.model_info / write_models_info / check_models_info apply them to a BOP tree."""
from __future__ import annotations

import math
from typing import Dict

import torch

from . import _lib
from .runtime import h2d, ptr, stream_ptr

EXTENT_R = 256        # kExtRows of csrc/models.hip: the pair walk's row tile (vertices a block holds in registers)
EXTENT_C = 1024       # kExtCols: its column tile (vertices staged in LDS)
RESIDUAL_R = 256      # kResRows: the residual's vertex tile
RESIDUAL_C = 256      # kResFaces: its face tile
SURFACE_TILE = 256    # kSurfTile of csrc/surface.hip: the faces per tile of the cumulative weights
FPS_MAX = 16384       # krrn_fps_f32's limit on the points of a set (csrc/fps.hip)


def _ranges(r: torch.Tensor, n: int):
    """A [n, 2] range tensor's host copy (for the callers' bounds: one read-back when it lives on the device)."""
    return r.reshape(n, 2).to("cpu", torch.int64)


def extent(verts: torch.Tensor, vert_range: torch.Tensor) -> Dict[str, torch.Tensor]:
    """krrn_model_extent_f64 for O objects in one call. verts [Vtot, 3] is a GPU tensor in any unit; vert_range [O, 2]
    = (first vertex, count) may be a host tensor (staged here). Returns host f64 tensors {"d2" [O] the squared
    diameter, "diameter" [O] = sqrt(d2), "min" [O, 3], "max" [O, 3], "size" [O, 3] = max - min}; an empty (or bad) range
    gives d2 = 0, min = +inf, max = -inf and size = -inf. An object's values do not depend on what else is in the call,
    bit for bit."""
    if not verts.is_cuda:
        raise RuntimeError("extent runs on the HIP path only (verts must be a GPU tensor)")
    dev = verts.device
    O = int(vert_range.reshape(-1, 2).shape[0])
    v = verts.to(torch.float32).contiguous()
    max_v = max(1, int(_ranges(vert_range, O)[:, 1].max())) if O else 1
    vr = h2d(vert_range.reshape(O, 2), dev, torch.int32)
    d2 = torch.empty((O,), dtype=torch.float64, device=dev)
    box = torch.empty((O, 6), dtype=torch.float64, device=dev)
    _lib.call("krrn_model_extent_f64", ptr(v), v.shape[0], ptr(vr), O, max_v, ptr(d2), ptr(box), stream_ptr(dev))
    d2, box = d2.cpu(), box.cpu()
    return {"d2": d2, "diameter": torch.tensor([math.sqrt(x) for x in d2.tolist()], dtype=torch.float64),
            "min": box[:, :3].clone(), "max": box[:, 3:].clone(), "size": box[:, 3:] - box[:, :3]}


def symmetry_residual(verts: torch.Tensor, faces: torch.Tensor, vert_range: torch.Tensor, face_range: torch.Tensor,
                      syms: torch.Tensor, sym_range: torch.Tensor, squared: bool = False) -> torch.Tensor:
    """krrn_symmetry_residual_f64 for O objects in one call: verts [Vtot, 3] / faces [Ftot, 3] (indices into verts) are
    GPU tensors; vert_range / face_range / sym_range [O, 2] and syms [NStot, 12] (bop.symmetry_set rows, concatenated
    over the objects, translations in the vertices' unit) may be host tensors. Returns host f64 [NStot] = sqrt(res2),
    in the vertices' unit: +inf for a NaN vertex or for vertices without faces, 0 for an object without vertices, NaN
    for a symmetry that no object's range owns. squared=True returns res2 itself, as the kernel stored it."""
    if not (verts.is_cuda and faces.is_cuda):
        raise RuntimeError("symmetry_residual runs on the HIP path only (verts / faces must be GPU tensors)")
    dev = verts.device
    O = int(vert_range.reshape(-1, 2).shape[0])
    v = verts.to(torch.float32).contiguous()
    f = faces.to(torch.int32).contiguous()
    max_v = max(1, int(_ranges(vert_range, O)[:, 1].max())) if O else 1
    max_f = max(1, int(_ranges(face_range, O)[:, 1].max())) if O else 1
    vr = h2d(vert_range.reshape(O, 2), dev, torch.int32)
    fr = h2d(face_range.reshape(O, 2), dev, torch.int32)
    sr = h2d(sym_range.reshape(O, 2), dev, torch.int32)
    sy = h2d(syms.reshape(-1, 12), dev, torch.float64)
    res2 = torch.full((sy.shape[0],), float("nan"), dtype=torch.float64, device=dev)
    _lib.call("krrn_symmetry_residual_f64", ptr(v), v.shape[0], ptr(f) if f.shape[0] else ptr(None), f.shape[0], ptr(vr),
              ptr(fr), ptr(sy), sy.shape[0], ptr(sr), O, max_v, max_f, ptr(res2), stream_ptr(dev))
    res2 = res2.cpu()
    if squared:
        return res2
    return torch.tensor([math.sqrt(x) if x == x else x for x in res2.tolist()], dtype=torch.float64)


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, face_range: torch.Tensor, n: int, seed: int = 0,
                   stream: int = 0, row_id=None, oversample: int = 1) -> Dict[str, torch.Tensor]:
    """krrn_surface_sample_f64 for O objects in one call: n points per object drawn uniformly on its surface (a face
    with probability proportional to its area, then the square-root barycentric map of the reference's
    tools/script/sample_model.py random_point), with the chosen face and its flat unit normal. verts [Vtot, 3] / faces
    [Ftot, 3] (indices into verts) are GPU tensors in any unit; face_range [O, 2] = (first face, count) may be a host
    tensor; row_id [O] (default 0..O-1) is each object's generator row: an object's samples depend on (seed, stream,
    its row) and its own faces only, not on what else is in the call. Returns GPU tensors {"points", "normals" f32
    [O, n, 3], "face" i32 [O, n] numbered within the object's range, "status" i32 [O]: 0, or 1 for an object without
    area (an empty or bad range, only degenerate faces), which keeps points = normals = 0 and face = -1, "area" f64
    [O]: the object's surface area, half the total weight}.

    oversample = k > 1 draws n * k candidates the same way and keeps the n that farthest point sampling picks from
    their f32 points (fps.farthest_point_sampling: from candidate 0, ties to the lowest index): the reference script's
    sampling followed by its FPS. Points, normals and faces are gathered by the FPS indices; an object with status !=
    0 does not enter the FPS. n * k above the FPS kernel's 16384 raises ValueError before anything runs."""
    n, k = int(n), int(oversample)
    if n < 1 or k < 1:
        raise ValueError(f"sample_surface needs n >= 1 and oversample >= 1, got n = {n}, oversample = {k}")
    if k > 1 and n * k > FPS_MAX:
        raise ValueError(f"n * oversample = {n * k} candidates exceed the FPS kernel's {FPS_MAX}")
    if not (verts.is_cuda and faces.is_cuda):
        raise RuntimeError("sample_surface runs on the HIP path only (verts / faces must be GPU tensors)")
    dev = verts.device
    O = int(face_range.reshape(-1, 2).shape[0])
    v = verts.to(torch.float32).contiguous()
    f = faces.to(torch.int32).contiguous()
    Ftot = int(f.shape[0])
    fr_host = _ranges(face_range, O)
    max_f = max(1, min(int(fr_host[:, 1].max()), Ftot)) if O else 1   # a count above Ftot is a bad range anyway
    fr = h2d(face_range.reshape(O, 2), dev, torch.int32)
    rows = torch.arange(O, dtype=torch.int32) if row_id is None else torch.as_tensor(row_id).reshape(O)
    if O and int(rows.min()) < 0:
        raise ValueError("row_id must be >= 0")
    rows = h2d(rows, dev, torch.int32)
    m = n * k
    cum = torch.zeros((O, max_f), dtype=torch.float64, device=dev)
    pts = torch.empty((O, m, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((O, m, 3), dtype=torch.float32, device=dev)
    face = torch.empty((O, m), dtype=torch.int32, device=dev)
    status = torch.empty((O,), dtype=torch.int32, device=dev)
    _lib.call("krrn_surface_sample_f64", ptr(v), v.shape[0], ptr(f) if Ftot else ptr(None), Ftot, ptr(fr), ptr(rows), O,
              max_f, m, int(seed), int(stream) & 0xFFFFFFFF, ptr(cum), ptr(pts), ptr(nrm), ptr(face), ptr(status),
              stream_ptr(dev))
    # the guarded face count, as the kernels take it (csrc/krrn_range.h), for total = cum[F - 1]
    first, cnt = fr_host[:, 0], fr_host[:, 1]
    nf = torch.where((first >= 0) & (cnt >= 0) & (cnt <= max_f) & (first + cnt <= Ftot), cnt, torch.zeros_like(cnt))
    last = h2d((nf - 1).clamp(min=0).reshape(O, 1), dev, torch.int64)
    area = torch.where(h2d(nf > 0, dev), cum.gather(1, last).reshape(O), torch.zeros((), dtype=torch.float64, device=dev)) / 2
    out = {"points": pts, "normals": nrm, "face": face, "status": status, "area": area}
    if k == 1:
        return out
    good = (status == 0).nonzero().reshape(-1)   # one read-back: the objects that enter the FPS
    G = int(good.shape[0])
    kept = {"points": torch.zeros((O, n, 3), dtype=torch.float32, device=dev),
            "normals": torch.zeros((O, n, 3), dtype=torch.float32, device=dev),
            "face": torch.full((O, n), -1, dtype=torch.int32, device=dev)}
    if G:
        cand = pts[good].contiguous()
        idx = torch.empty((G, n), dtype=torch.int32, device=dev)
        _lib.call("krrn_fps_f32", ptr(cand), G, m, n, ptr(idx), stream_ptr(dev))
        for key, src, w in (("points", cand, 3), ("normals", nrm[good].contiguous(), 3),
                            ("face", face[good].contiguous().view(torch.float32), 1)):  # 32-bit rows, copied as they are
            dst = torch.empty((G, n, w), dtype=torch.float32, device=dev)
            _lib.call("krrn_gather_rows_f32", ptr(idx), 0, n, n, ptr(src), m * w, w, ptr(dst), n * w, w, w, G,
                      stream_ptr(dev))
            kept[key][good] = dst if w == 3 else dst.view(torch.int32).reshape(G, n)
    out.update(kept)
    return out
