"""Translation head of KRRN (lib/network/pose/posenet.py:51-96), MI355X execution.

TBase = Conv1d(1280 + C -> 1024) + BN + ReLU -> (-> 256) + BN + ReLU -> (-> 256) + BN + ReLU
        -> Dropout (eval: identity) -> Conv1d(-> OUT_T); t_res = [:, 0:3]
and KRRN.forward's pred_t = mean_N(p_emb + t_res) (krrn.py:153).

Execution: the one-hot class channels of the concat (krrn.py:132-138) contribute exactly the
column W1[:, 1280 + cls] to conv1, so they become a per-crop bias (one gather launch) instead
of C extra input channels; conv1 runs by linearity on the fusion's level rows (see
build_tbase_plan); conv1..conv3 are f32-MFMA GEMMs with BN folded into the epilogue;
conv4 + the mean over points is one reduction launch per crop.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import knobs, ops
from .runtime import Late, Plan, add_gemm, ptr


# conv2 / conv3 once per distinct (nn1, nn2) pair of a crop (h1's row is a function of the pair only;
# ~36 % of the points at config 2), the tail reads each point's row by its slot; 0 = once per point
TBASE_DISTINCT = knobs.flag("KRRN_TBASE_DISTINCT")
PAIR_MAX_KEYS = 1 << 18  # krrn_pair_compact_i32's LDS key bitmap (N1 * N2 of config 5: 1024 x 256)


class TBase(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.f = cfg.Module.POSENet.INC_R + cfg.Module.NUM_CLS
        self.k = cfg.Module.POSENet.OUT_T
        self.conv1 = nn.Conv1d(self.f, 1024, 1)
        self.conv2 = nn.Conv1d(1024, 256, 1)
        self.conv3 = nn.Conv1d(256, 256, 1)
        self.conv4 = nn.Conv1d(256, self.k, 1)
        self.drop1 = nn.Dropout(0.2)
        self.bn1 = nn.BatchNorm1d(1024)
        self.bn2 = nn.BatchNorm1d(256)
        self.bn3 = nn.BatchNorm1d(256)


class PoseNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.t_net = TBase(cfg)


def _conv1_fold(tb: TBase, inc_r: int, num_cls: int, dev):
    """conv1 + bn1 folded: (W1 [1024, inc_r + C], spec1 with the BN scale / bias, colv [C, 1024] =
    the one-hot columns pre-multiplied by the BN scale)."""
    w1 = tb.conv1.weight.detach()[:, :, 0]
    spec1 = ops.make_linear(w1[:, :inc_r], tb.conv1.bias, tb.bn1, dev)
    np1 = ops.pad4(1024)
    colv = torch.zeros(num_cls, np1, device=dev)
    colv[:, :1024] = (spec1.scale[:1024, None] * w1[:, inc_r:inc_r + num_cls].to(dev).float()).t()
    return w1, spec1, colv


NEEDS_X3 = "TBase's GEMMs need the split-bf16 GEMM, which does not take this shape (runtime.add_gemm)"


def emit_tbase_level1(tb: TBase, plan: Plan, B: int, N: int, N1: int, feat1: torch.Tensor,
                      feat2: torch.Tensor, cls_key: str = "cls", inc_r: int = 1280, num_cls: int = 1) -> dict:
    """The part of TBase conv1 (by linearity, see build_tbase_plan) that needs only the level-0 /
    level-1 features: P1 = feat1[:N1] W1[:, 512:896]^T + feat2 W1[:, 896:1280]^T, on the plan's
    current stream. Emitted from the fusion's 'level1' hook, it runs beside the level-2 GCN chain.
    The BN scale is folded into those weights and the BN shift + conv1 bias + the crop's one-hot
    column are added here, so conv2 only has to gather, add and ReLU (fused into its operand staging,
    krrn_gemm_x3_gather_f32)."""
    dev = plan.device
    np1 = ops.pad4(1024)
    w1, spec1, colv = _conv1_fold(tb, inc_r, num_cls, dev)
    wb = ops.make_linear(w1[:, 512:896], None, None, dev)
    wc = ops.make_linear(w1[:, 896:1280], None, None, dev)
    b2 = plan.buf((B, np1))
    plan.add("krrn_gather_rows_f32", Late(cls_key), 1, 1, 1, ptr(colv), 0, np1, ptr(b2), np1, np1, np1, B)
    Q = plan.buf((B * N1, np1))
    P1 = plan.buf((B * N1, np1))
    # Q = s (feat2 Wc) + shift + b2[crop] (the crop's row of b2 broadcast: ldr = 0, one row per group)
    ok = add_gemm(plan, a=feat2, a_off=0, lda=384, M=N1, wt=wc.wt[0], K=wc.cin_p, N=np1, scale=spec1.scale,
                  bias=spec1.bias, out=Q, ldo=np1, relu=False, res=b2, ldr=0, batch=B, a_grp=N1 * 384,
                  o_grp=N1 * np1, r_grp=np1, cin=wc.cin, cout=wc.cout, tag="tbase_gemm", require_x3=True) and \
        add_gemm(plan, a=feat1, a_off=0, lda=384, M=N1, wt=wb.wt[0], K=wb.cin_p, N=np1, scale=spec1.scale,
                 bias=None, out=P1, ldo=np1, relu=False, res=Q, ldr=np1, batch=B, a_grp=N * 384,
                 o_grp=N1 * np1, r_grp=N1 * np1, cin=wb.cin, cout=wb.cout, tag="tbase_gemm", require_x3=True)
    if not ok:
        raise RuntimeError(NEEDS_X3)
    plan.buffers.append([wb, wc, spec1, colv])
    return dict(P1=P1, Q=Q, b2=b2)


def emit_pair_compact(plan: Plan, B: int, N: int, N1: int, N2: int, nn1: torch.Tensor,
                      nn2: torch.Tensor) -> Optional[dict]:
    """The distinct (nn1, nn2) pairs of every crop, on the plan's current stream: cnt [B], the pairs
    pa / pb [B, N] in ascending key order (entries past cnt repeat entry 0) and each point's slot
    [B, N] (krrn_pair_compact_i32). It needs only the two nearest-index buffers, so the fusion emits
    it right behind them. None when TBase runs per point: the knob, or a shape past the kernel's
    limits (it would return KRRN_ESHAPE)."""
    if not TBASE_DISTINCT or N1 * N2 > PAIR_MAX_KEYS or N > 0xFFFF:
        return None
    i32 = torch.int32
    pr = dict(cnt=plan.buf((B,), i32), pa=plan.buf((B, N), i32), pb=plan.buf((B, N), i32), slot=plan.buf((B, N), i32))
    plan.add("krrn_pair_compact_i32", ptr(nn1), ptr(nn2), B, N, N1, N2, ptr(pr["cnt"]), ptr(pr["pa"]), ptr(pr["pb"]),
             ptr(pr["slot"]))
    return pr


def build_tbase_plan(tb: TBase, plan: Plan, B: int, N: int, cls_key: str, cloud_key: str, inc_r: int, num_cls: int,
                     levels: dict, pre: Optional[dict] = None, pre_sid: int = 0, pairs: Optional[dict] = None):
    """Emit TBase + pred_t. cls ([B, 1] int64) and cloud ([B, N, 3]) are late-bound env tensors.
    Returns the [B, 3] pred_t buffer and the intermediate buffers.

    `levels`: the fusion's level rows fm5 [B, N2, 512], feat1 [B, N, 384], feat2 [B, N1, 384], the
    nearest indices nn1 / nn2 that build the 1280-wide concat (fusion.py:230-238) and N1 / N2. conv1
    runs by linearity on the level rows instead of the N gathered rows: P2 = fm5 W1[:, :512]^T (N2
    rows), P1 = feat1[:N1] W1[:, 512:896]^T + feat2 W1[:, 896:1280]^T (N1 rows; the reference indexes
    feat_1 with nearest_pool_1, so only its first N1 rows are ever read), both with BN, bias and the
    one-hot column folded in (emit_tbase_level1); conv2 builds h1 = ReLU(P1[nn1] + P2[nn2]) in its
    operand staging, so h1 is never in HBM. 29 instead of 168 GFLOP at config 2.
    `pre`: P1 already emitted by emit_tbase_level1 on stream `pre_sid` (joined here before use).

    Two forms. Per point: conv2 / conv3 on all B * N rows, the tail sums them in order. Per distinct
    pair (KRRN_TBASE_DISTINCT and a shape within emit_pair_compact's limits; `pairs` = its buffers
    when the fusion emitted it already, on a stream joined before this): h2 and h3 keep their
    [B*N, 256] shape, but rows j < cnt[b] of crop b hold the rows of the crop's distinct (nn1, nn2)
    pairs in key order (rows past the last live 128-row tile are never written), and the tail reads
    point i's row at slot[b, i]. Every row is the per-point form's row bit for bit, and so is pred_t.
    The ops' meta keeps the per-point FLOP count (the algorithmic work)."""
    dev = plan.device
    w1, spec1, _ = _conv1_fold(tb, inc_r, num_cls, dev)
    np1 = ops.pad4(1024)
    spec2 = ops.make_linear(tb.conv2.weight, tb.conv2.bias, tb.bn2, dev)
    spec3 = ops.make_linear(tb.conv3.weight, tb.conv3.bias, tb.bn3, dev)
    w4 = tb.conv4.weight.detach()[:3, :, 0].float().contiguous().to(dev)
    b4 = tb.conv4.bias.detach()[:3].float().contiguous().to(dev)
    N1, N2 = levels["N1"], levels["N2"]
    if pairs is None:  # straight after nn1 / nn2 (the fusion joined their stream)
        pairs = emit_pair_compact(plan, B, N, N1, N2, levels["nn1"], levels["nn2"])
    h2 = plan.buf((B * N, 256))
    h3 = plan.buf((B * N, 256))
    pred_t = plan.buf((B, 3))
    M = B * N
    wa = ops.make_linear(w1[:, 0:512], None, None, dev)
    P2 = plan.buf((B * N2, np1))
    # BN scale folded into W1's columns, as for P1 (emit_tbase_level1)
    if not add_gemm(plan, a=levels["fm5"], a_off=0, lda=512, M=B * N2, wt=wa.wt[0], K=wa.cin_p, N=np1,
                    scale=spec1.scale, bias=None, out=P2, ldo=np1, relu=False, cin=wa.cin, cout=wa.cout,
                    tag="tbase_gemm", require_x3=True):
        raise RuntimeError(NEEDS_X3)
    if pre is None:
        pre = emit_tbase_level1(tb, plan, B, N, N1, levels["feat1"], levels["feat2"], cls_key=cls_key,
                                inc_r=inc_r, num_cls=num_cls)
    else:
        plan.join([pre_sid])
    P1 = pre["P1"]
    # conv2 with h1 = ReLU(P1[nn1] + P2[nn2]) built in its operand staging, conv3 (on the live rows of
    # every crop: one group of N rows per crop) and the tail (by slot)
    w2 = tb.conv2.weight.detach()[:, :, 0].to(dev).float() * spec2.scale[:256].reshape(256, 1)
    w3 = ops.gemm_weights_x3(w2.contiguous())
    meta = dict(kernel="gemm_x3", flops=2.0 * 1024 * 256 * M, tag="tbase_gemm", M=M, N=256, K=1024,
                splits=1, mfma_flops=2.0 * M * 256 * 1024 * 6 / 16, mfma_bf16_flops=2.0 * M * 256 * 1024 * 6)
    conv3 = dict(a=h2, a_off=0, lda=256, wt=spec3.wt[0], K=spec3.cin_p, N=ops.pad4(spec3.cout), scale=spec3.scale,
                 bias=spec3.bias, out=h3, ldo=256, relu=True, cin=spec3.cin, cout=spec3.cout, tag="tbase_gemm",
                 require_x3=True)
    if pairs is not None:
        plan.add("krrn_gemm_x3_gather_live_f32", ptr(pairs["pa"]), ptr(P1), N1 * np1, np1, ptr(pairs["pb"]),
                 ptr(P2), N2 * np1, np1, N, B, 1024, 256, ptr(w3), ptr(spec2.bias), ptr(h2), 256, 1,
                 ptr(pairs["cnt"]), meta=meta)
        ok = add_gemm(plan, M=N, batch=B, a_grp=N * 256, o_grp=N * 256, live=pairs["cnt"], **conv3)
        tail = ("krrn_tbase_tail_slot_f32", ptr(h3), ptr(pairs["slot"]))
    else:
        plan.add("krrn_gemm_x3_gather_f32", ptr(levels["nn1"]), ptr(P1), N1 * np1, np1, ptr(levels["nn2"]),
                 ptr(P2), N2 * np1, np1, N, B, 1024, 256, ptr(w3), ptr(spec2.bias), ptr(h2), 256, 1, meta=meta)
        ok = add_gemm(plan, M=M, **conv3)
        tail = ("krrn_tbase_tail_f32", ptr(h3))
    if not ok:
        raise RuntimeError(NEEDS_X3)
    plan.add(*tail, B, N, 256, ptr(w4), ptr(b4), Late(cloud_key), ptr(pred_t), ptr(None))
    plan.buffers.append([spec1, spec2, spec3, w4, b4, wa, w3])
    return pred_t, dict(h2=h2, h3=h3, **(pairs or {}))
