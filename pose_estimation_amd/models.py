"""Object-model facts on the GPU: what BOP's calc_model_info script computes (the diameter and the axis-aligned box of
every model), and how well a declared symmetry maps a mesh onto itself (include/krrn_hip.h states both definitions,
tests/models_ref.py restates them in numpy).

    e = extent(verts, vert_range)
    # -> {"d2": f64 [O], "diameter": f64 [O] = sqrt(d2), "min", "max": f64 [O, 3], "size": f64 [O, 3] = max - min}, host values
    r = symmetry_residual(verts, faces, vert_range, face_range, syms, sym_range)
    # -> f64 [NStot], host values: per symmetry the largest distance from a transformed vertex to the surface

Both are in the vertices' own unit (the symmetries' translations too). The diameter is the maximum over all vertex
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
