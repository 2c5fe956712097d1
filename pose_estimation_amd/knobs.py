"""Every environment variable the package reads, declared once (name -> default, meaning).

The defaults are the shipped configuration; each knob selects a measured alternative that still
exists in the code (for A/B timing on the GPU box, DESIGN.md records the numbers) or sizes a
cache. The C-ABI library reads no environment at all: its tuning is fixed at build time.
Modules read knobs at import time through `flag` / `integer` / `text`, so a value must be set
before the package is imported. tests/test_knobs.py checks that nothing outside this table is read.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

KNOBS: Dict[str, Tuple[Optional[str], str]] = {
    # --- loading, execution, capacity
    "KRRN_HIP_LIB": (None, "path of the C-ABI library to load instead of the in-tree libkrrn_hip.so "
                           "(variant builds for A/B timing, the KRRN_DIAG diagnostics build)"),
    "KRRN_GRAPH": ("1", "KRRN.forward replays a captured hipGraph of its plan; 0 = serial eager runs"),
    "KRRN_PLAN_STREAMS": ("1", "captured plans keep their side streams as graph branches; 0 = captured serially"),
    "KRRN_STREAMS": ("1", "the two-slot pipeline's stages, concurrent micro-batches and config 3's buckets "
                          "replay side by side on their own streams; 0 = one after the other"),
    "KRRN_PLAN_BUDGET_GB": ("48", "device memory the KRRN plan cache may hold before evicting the least "
                                  "recently used (B, S, N) plan"),
    "KRRN_DIAG_DROP": ("", "comma list of C-ABI entry points left out of new plans: a what-if timing "
                           "diagnostic (profiles/whatif.sh); outputs are meaningless with it set"),
    # --- plan scheduling (each alternative is a kept, tested path; which kernel runs a conv or GEMM
    # is decided by shape eligibility alone: hrnet._Builder.conv, runtime.add_gemm)
    "KRRN_FUSE_EARLY": ("1", "HRNet fuse terms that read one branch start on that branch's stream before the join"),
    "KRRN_MODULE_STREAMS": ("1", "consecutive HRNet modules of a stage keep each branch on its stream (no barrier between them)"),
    "KRRN_STAGE_STREAMS": ("1", "with KRRN_MODULE_STREAMS, HRNet stages chain per branch stream too (transitions on their branch's stream)"),
    "KRRN_FUSION_EARLY": ("1", "the fusion work that reads only the input cloud runs beside the HRNet phase (side stream)"),
    "KRRN_FUSE_EDGES": ("1", "each HRNet fuse output waits for exactly its branches (capture edges); 0 = module barrier"),
    "KRRN_TBASE_EARLY": ("1", "TBase conv1's level-1 half runs as soon as level 1 is done (side stream)"),
    "KRRN_TBASE_DISTINCT": ("1", "TBase conv2 / conv3 run once per distinct (nn1, nn2) "
                                 "pair of a crop and the tail reads each point's row by its slot (same bits); "
                                 "0 = once per point"),
    "KRRN_POSE_AT": ("level1", "where the fused pose step forks off the forward plan: level1 / level2 / heads"),
    "KRRN_FUSION_CHUNK": ("16", "crops per chunk of the level-0 GCN GEMM + gather-conv, through a chunk-sized "
                                "Y buffer per branch (0 = the whole batch at once; same results)"),
}


def text(name: str) -> Optional[str]:
    if name not in KNOBS:
        raise KeyError(f"{name} is not a declared knob (pose_estimation_amd/knobs.py)")
    return os.environ.get(name, KNOBS[name][0])


def flag(name: str) -> bool:
    return text(name) == "1"


def integer(name: str) -> int:
    return int(text(name))
