"""f64 restatements of csrc/loss.hip's results and the edge inputs its GPU tests run (test
infrastructure: tests/test_loss_ref_host.py pins this file on the CPU, tests/test_gpu_loss.py uses it
unchanged against the kernels).

Map terms (krrn_map_losses_f32, krrn_map_losses_crop_f32): `map_terms` takes the f32 inputs to f64 and
returns each crop's four sums and valid counts; `pooled` / `per_crop` turn them into the kernel's two
outputs (sum / count, 0.0 where the count is 0). As in the kernel the 1e-6 inside the log and the
cosine's clamp are float32(1e-6), labels outside [0, C) are skipped, and a target pixel is valid when
any channel != 0 (so -0.0 in every channel is invalid).

Point terms (krrn_pose_loss_f32, krrn_add_metric_f32): `points_ref` gives, per crop, PoseLoss (per
prediction the min over targets for a symmetric crop), ADD and ADD-S (per target the min over
predictions), each the mean of sqrt(min d^2) so that index ties cannot change it. The same function
at dtype=float32 is the f32 torch restatement whose own error scales the GPU tolerance (`point_tol`).
"""
import numpy as np
import torch

EPS32 = float(np.float32(1e-6))
BLOCK = 4096  # kLossPixPerBlock: pixels of one crop per block of map_losses_kernel
QUERIES = 256  # kLossThreads: queries per block of pose_loss_kernel / add_metric_kernel
TILE = 2048  # kPoseTile: candidates staged per LDS tile
MAP_RTOL = 2e-6  # the project's tolerance for the map terms and ADD(-S) (tests/test_loss.py, test_metric.py)


# ---- map terms ---------------------------------------------------------------------------------
def _ce(x, lab):
    """x f64 [B, C, HW], lab int64 [B, HW] -> (-log(softmax(x)[lab] + float32(1e-6)) [B, HW], valid)."""
    C = x.shape[1]
    valid = (lab != 0) & (lab >= 0) & (lab < C)
    p = torch.softmax(x, 1).gather(1, lab.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    return -torch.log(p + EPS32), valid


def map_pixels(pred, gt):
    """Per-pixel loss f64 [4, B, HW] and validity bool [4, B, HW] of the four terms (xyz, normal,
    region, mask)."""
    B = pred["xyz"].shape[0]
    d = lambda t: t.double().reshape(B, t.shape[1], -1)  # noqa: E731
    x, t = d(pred["xyz"]), d(gt["xyz"])
    l1, v1 = (x - t).abs().sum(1), (t != 0).any(1)
    x, t = d(pred["normal"]), d(gt["normal"])
    nx, nt = x.norm(dim=1).clamp_min(EPS32), t.norm(dim=1).clamp_min(EPS32)
    cos, v2 = 1.0 - ((x / nx[:, None]) * (t / nt[:, None])).sum(1), (t != 0).any(1)
    ce_r, v3 = _ce(d(pred["region"]), gt["region"].long().reshape(B, -1))
    ce_m, v4 = _ce(d(pred["mask"]), gt["multi_cls_mask"].long().reshape(B, -1))
    return torch.stack([l1, cos, ce_r, ce_m]), torch.stack([v1, v2, v3, v4])


def map_terms(pred, gt):
    """(sums f64 [B, 4], counts int64 [B, 4]) per crop."""
    loss, valid = map_pixels(pred, gt)
    return (loss * valid).sum(2).t().contiguous(), valid.sum(2).t().contiguous()


def _ratio(s, n):
    return torch.where(n > 0, s / n.clamp_min(1).double(), torch.zeros_like(s))


def pooled(sums, counts):
    """The kernel's out[0..3] and out[4..7]: valid pixels pooled over the batch."""
    return _ratio(sums.sum(0), counts.sum(0)), counts.sum(0)


def per_crop(sums, counts):
    """The per-crop kernel's out[b][0..3] and out[b][4..7]."""
    return _ratio(sums, counts), counts


def block_records(pred, gt):
    """(sums [B, nbx, 4], counts [B, nbx, 4]): the partial records map_losses_kernel leaves, one per
    4096-pixel block of each crop, for the mutation checks on the reducers' indexing."""
    loss, valid = map_pixels(pred, gt)
    HW = loss.shape[2]
    nbx = -(-HW // BLOCK)
    pad = nbx * BLOCK - HW
    f = lambda a: torch.nn.functional.pad(a, (0, pad)).reshape(4, a.shape[1], nbx, BLOCK)  # noqa: E731
    s = f(loss * valid).sum(3).permute(1, 2, 0).contiguous()
    n = f(valid.long()).sum(3).permute(1, 2, 0).contiguous()
    return s, n


def boundary_pixels(HW):
    """First and last pixel of every 4096-pixel block, and pixel HW - 1."""
    out = set()
    for p0 in range(0, HW, BLOCK):
        out |= {p0, min(HW, p0 + BLOCK) - 1}
    return sorted(out)


def empty_block(B, HW):
    """(crop, block) left without a valid pixel by edge_maps, or None when a crop has one block."""
    nbx = -(-HW // BLOCK)
    return (1, nbx - 2) if nbx > 1 and B > 1 else None


def edge_maps(B, H, W, R, M, seed):
    """Maps whose block and crop structure shows in the result (pred, gt as tests/test_loss._maps).

    Valid fraction about 0.6. Crop b's xyz prediction is offset by b. The boundary pixels
    (`boundary_pixels`) are valid for all four terms in every crop and carry at least 20 x the crop's
    typical per-pixel loss, so a block that drops or doubles its first or last pixel moves the mean
    far more than the tolerance. The largest per-pixel values the terms allow set the typical ones:
    1 - cosine <= 2, so predicted normals are the target plus noise (sigma 0.22 to 0.28 by crop:
    typical 1 - cos 0.05 to 0.08; smaller would leave f32 rounding of a cosine near 1 a visible part of
    the mean) and a boundary pixel's is nearly opposite (1.9 to 2.0); -log(p + 1e-6) <= 13.8, so the
    logits are noise plus a boost at the label (typical CE 0.04 to 0.2), scaled by 1 + (b % 4) / 6 so
    that crops differ (a scale of 1 + b would push the typical CE of later crops to the 13.8 cap or to
    0), and a boundary pixel's label sits 10 to 12 under another class. Boundary values are drawn per
    pixel, so that no two crops' records hold the same ones. Crop 1's block
    `empty_block` has no valid pixel for any term (with two blocks that leaves the crop its last pixel
    alone); crop B - 1 has no valid mask label at all."""
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    valid = torch.rand(B, HW, generator=g) < 0.6
    bp = torch.tensor(boundary_pixels(HW))
    valid[:, bp] = True
    eb = empty_block(B, HW)
    if eb is not None:
        valid[eb[0], eb[1] * BLOCK:min(HW, (eb[1] + 1) * BLOCK)] = False
    crop = torch.arange(B, dtype=torch.float32)
    gt_xyz = (0.05 + torch.rand(B, 3, HW, generator=g)) * valid[:, None]
    xyz = torch.rand(B, 3, HW, generator=g) + crop.view(B, 1, 1)
    gt_n = torch.nn.functional.normalize(rn(B, 3, HW), dim=1) * valid[:, None]
    sigma = 0.22 + 0.03 * (crop % 3)
    nml = (gt_n + sigma.view(B, 1, 1) * rn(B, 3, HW)) * (0.5 + torch.rand(B, 1, HW, generator=g))
    nml = torch.where(valid[:, None], nml, rn(B, 3, HW))
    scale = 1.0 + (crop % 4) / 6.0
    maps = {}
    for key, C in (("region", R), ("mask", M)):
        lab = torch.randint(1, C, (B, HW), generator=g) * valid
        boost = float(np.log(C)) + 2.5
        x = rn(B, C, HW) + boost * torch.nn.functional.one_hot(lab, C).permute(0, 2, 1) * valid[:, None]
        maps[key] = (scale.view(B, 1, 1) * x, lab)
    # the boundary pixels: typical l1 of crop b is about 3 b + 1
    sign = torch.tensor([1.0, -1.0, 1.0]).view(1, 3, 1)
    big = (25.0 * (3.0 * crop + 1.0) / 3.0).view(B, 1, 1)
    live = valid[:, bp]  # all True except inside the empty block
    xyz[:, :, bp] = torch.where(live[:, None], gt_xyz[:, :, bp] + sign * big, xyz[:, :, bp])
    nml[:, :, bp] = torch.where(live[:, None], -1.7 * gt_n[:, :, bp] + 0.3 * rn(B, 3, len(bp)), nml[:, :, bp])
    for key, C in (("region", R), ("mask", M)):
        x, lab = maps[key]
        xb = x[:, :, bp]
        hot = torch.nn.functional.one_hot(lab[:, bp], C).permute(0, 2, 1).bool()
        other = torch.nn.functional.one_hot((lab[:, bp] + 1) % C, C).permute(0, 2, 1).bool()
        u = 5.0 + torch.rand(B, 1, len(bp), generator=g)  # CE about 2 u, another value at every pixel
        xb = torch.where(hot, -u, torch.where(other, u, xb))
        x[:, :, bp] = torch.where(live[:, None], xb, x[:, :, bp])
    maps["mask"][1][B - 1] = 0
    pred = {"xyz": xyz.view(B, 3, H, W), "normal": nml.view(B, 3, H, W),
            "region": maps["region"][0].view(B, R, H, W), "mask": maps["mask"][0].view(B, M, H, W)}
    gt = {"xyz": gt_xyz.view(B, 3, H, W), "normal": gt_n.view(B, 3, H, W),
          "region": maps["region"][1].view(B, H, W), "multi_cls_mask": maps["mask"][1].view(B, H, W)}
    return pred, gt


def invalidate(gt, b, p):
    """A copy of gt with pixel p of crop b invalid for all four terms (the mutation 'a block dropped
    this pixel')."""
    out = {k: v.clone() for k, v in gt.items()}
    for k in ("xyz", "normal"):
        out[k].view(out[k].shape[0], 3, -1)[b, :, p] = 0.0
    for k in ("region", "multi_cls_mask"):
        out[k].view(out[k].shape[0], -1)[b, p] = 0
    return out


def branch_maps(empty_mask=False):
    """One small batch (B, H, W, R, M = 2, 6, 7, 5, 3) that takes every branch of the map kernel
    the random maps do not: logits of +-90 in both maps (expf overflows without the max subtraction),
    a labelled class whose probability underflows to 0 (-log(1e-6)) and one whose probability is 1
    (-log(1 + 1e-6) < 0), a zero predicted normal at a valid pixel (the 1e-6 clamp on the prediction),
    a 1e-9 normal target (the clamp on the target), -0.0 in every channel of an xyz and a normal
    target pixel (invalid), labels -1 and C (skipped, not counted), and the xyz target zero (+0.0 and
    -0.0) everywhere: that term is empty for the whole batch, 0.0 with count 0. empty_mask=True
    empties the mask term as well."""
    B, H, W, R, M = 2, 6, 7, 5, 3
    g = torch.Generator().manual_seed(77)
    HW = H * W
    valid = torch.rand(B, HW, generator=g) < 0.6
    valid[:, :8] = True
    pred = {"xyz": torch.rand(B, 3, HW, generator=g), "normal": torch.randn(B, 3, HW, generator=g),
            "region": 3 * torch.randn(B, R, HW, generator=g), "mask": 3 * torch.randn(B, M, HW, generator=g)}
    gt = {"xyz": torch.zeros(B, 3, HW),
          "normal": torch.nn.functional.normalize(torch.randn(B, 3, HW, generator=g), dim=1) * valid[:, None],
          "region": torch.randint(1, R, (B, HW), generator=g) * valid,
          "multi_cls_mask": torch.randint(1, M, (B, HW), generator=g) * valid}
    gt["xyz"][:, :, ::3] = -0.0
    pred["normal"][0, :, 1] = 0.0
    gt["normal"][0, :, 2] = torch.tensor([0.0, 0.0, 1e-9])
    gt["normal"][1, :, 3] = -0.0
    for key, lab_key, C in (("region", "region", R), ("mask", "multi_cls_mask", M)):
        x, lab = pred[key], gt[lab_key]
        x[0, :, 4], lab[0, 4] = -90.0, 1
        x[0, 0, 4] = 90.0  # label 1 at -90 under a +90: probability underflows
        x[1, :, 5], lab[1, 5] = -90.0, C - 1
        x[1, C - 1, 5] = 90.0  # the label itself at +90: probability 1
        lab[0, 6], lab[1, 7] = -1, C
    if empty_mask:
        gt["multi_cls_mask"][:] = 0
    sh = lambda t: t.view(B, -1, H, W) if t.dim() == 3 else t.view(B, H, W)  # noqa: E731
    return {k: sh(v) for k, v in pred.items()}, {k: sh(v) for k, v in gt.items()}


# ---- point terms -------------------------------------------------------------------------------
def _nearest(q, c, chunk=512):
    """sqrt of the min over candidates c [P, 3] of the squared distance, per query q [Q, 3]."""
    out = torch.empty(q.shape[0], dtype=q.dtype)
    for i in range(0, q.shape[0], chunk):
        d = q[i:i + chunk, None, :] - c[None, :, :]
        out[i:i + chunk] = (d * d).sum(-1).min(1)[0].sqrt()
    return out


def points_ref(R, t, mp, target, sym_mask, dtype=torch.float64, terms=("pose", "adds")):
    """Per crop, in `dtype` from the f32 inputs (results as f64 [B]):
      pose: PoseLoss's term, mean_i |pred_i - target_i|, or for a symmetric crop mean over
            predictions i of min over targets j |pred_i - target_j|;
      add:  mean_i |pred_i - target_i|;
      adds: mean over targets i of min over predictions j |pred_j - target_i| (ADD-S).
    krrn_pose_loss_f32 returns pose.mean(); krrn_add_metric_f32 returns adds for a symmetric crop and
    add otherwise (`add_metric_ref`). `terms`: which of the two searches to run (the other key then
    holds add)."""
    R, t, mp, target = (a.to(dtype) for a in (R, t, mp, target))
    B = mp.shape[0]
    pred = mp @ R.reshape(B, 3, 3).transpose(1, 2) + t.reshape(B, 1, 3)
    add = (pred - target).norm(dim=2).mean(1).double()
    pose, adds = add.clone(), add.clone()
    for b in range(B):
        if sym_mask[b] and "pose" in terms:
            pose[b] = _nearest(pred[b], target[b]).double().mean()
        if sym_mask[b] and "adds" in terms:
            adds[b] = _nearest(target[b], pred[b]).double().mean()
    return {"pose": pose, "add": add, "adds": adds}


def add_metric_ref(ref, sym_mask):
    return torch.where(torch.as_tensor(sym_mask), ref["adds"], ref["add"])


def point_tol(ref64, ref32, max_coord):
    """The bound on |kernel - f64|, per value: the largest of 4 x the f32 restatement's own error
    (the kernel contracts FMAs and orders its sums differently), 8 * 2^-24 * max |coordinate| (three
    products and three adds per coordinate at that magnitude, three coordinates, then the difference
    and the norm), and 2e-6 relative."""
    ref64, ref32 = torch.as_tensor(ref64).double(), torch.as_tensor(ref32).double()
    return torch.maximum(torch.maximum(4 * (ref32 - ref64).abs(), torch.full_like(ref64, 8 * 2.0**-24 * max_coord)),
                         MAP_RTOL * ref64.abs())


def max_coord(R, t, mp, target):
    B = mp.shape[0]
    pred = mp.double() @ R.double().reshape(B, 3, 3).transpose(1, 2) + t.double().reshape(B, 1, 3)
    return float(max(pred.abs().max(), target.abs().max(), mp.abs().max()))


def special_indices(P):
    """(S, T): the block- and tile-edge indices 0, 255, 256, 2047, 2048, P - 1 that exist (queries
    of a 256-thread block's first and last lane, candidates at a 2048-point tile's ends), and the
    tile-edge ones among them."""
    S = sorted({i for i in (0, QUERIES - 1, QUERIES, TILE - 1, TILE, P - 1) if 0 <= i < P})
    T = sorted({i for i in (0, TILE - 1, TILE, P - 1) if 0 <= i < P})
    return S, T


STATION_D = 6.0  # metres from the object to a station; stations are sqrt(2) x that apart
EXTRA = 0.9  # an extra query sits 0.9 x STATION_D from its station's candidate


def edge_points(B, P, sym_mask, seed):
    """(R [B, 3, 3], pred_t [B, 3], mp [B, P, 3], target [B, P, 3]), f32.

    Model points in a +-0.06 m box, random rotations, t about (0, 0, 0.9), the predicted t off by
    0.01 per axis (sigma). A non-symmetric crop's targets are its model points under the exact pose.
    A symmetric crop's targets are a different point set: an independent draw over half the box
    (+-0.03 m), transformed, so that 'nearest target per prediction' (PoseLoss; large for predictions
    outside the targets' hull) and 'nearest prediction per target' (ADD-S) are far apart and a
    swapped direction shows.

    In a symmetric crop the points at `special_indices` of both sets are moved out to stations
    STATION_D from the object (on the +-x and +-y axes of the camera frame, 8.5 m apart), one
    station per tile-edge index j of T: it holds target j and the prediction at the next tile-edge
    index (a cyclic shift, so no pair shares its index), about 1 cm apart. Every such point's only
    near neighbour in the other set is therefore that set's point at a tile-edge index, first or last
    of an LDS tile: a tile loop that misses its first or last candidate, or a block that misses its
    first or last query, changes the mean by metres / P (metres, because the tolerance carries
    8 * 2^-24 * max |coordinate| and P reaches 4097). The block-edge indices that are no tile edge
    (255, 256) go 5.4 m above (predictions) or below (targets) a station: still nearer its tile-edge
    point of the other set than anything else (>= 8 m), and far enough that the station's own pair
    stays each other's nearest. Isolation is between the two sets, which is all a nearest search
    between them sees."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    box = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    mp = box(B, P, 3) * 0.12
    Rs = torch.linalg.qr(rn(B, 3, 3))[0]
    Rs = Rs * torch.sign(torch.det(Rs)).view(B, 1, 1)
    t = 0.05 * rn(B, 3) + torch.tensor([0.0, 0.0, 0.9], dtype=torch.float64)
    pred_t = t + 0.01 * rn(B, 3)
    Rs, t, pred_t = Rs.float().double(), t.float().double(), pred_t.float().double()
    target = mp @ Rs.transpose(1, 2) + t[:, None]
    S, T = special_indices(P)
    extras = [i for i in S if i not in T]
    centres = STATION_D * torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0]], dtype=torch.float64)
    up = torch.tensor([0.0, 0.0, EXTRA * STATION_D], dtype=torch.float64)
    for b in range(B):
        if not sym_mask[b]:
            continue
        target[b] = (box(P, 3) * 0.06) @ Rs[b].T + t[b]
        cam = mp[b] @ Rs[b].T + pred_t[b]  # the predictions, camera frame
        for k, j in enumerate(T):
            c = centres[k] + t[b]
            target[b, j] = c
            cam[T[(k + 1) % len(T)]] = c + 0.01 * torch.nn.functional.normalize(rn(3), dim=0)
        for k, i in enumerate(extras):
            cam[i] = centres[k % len(T)] + t[b] + up + 0.01 * rn(3)
            target[b, i] = centres[(k + 1) % len(T)] + t[b] - up + 0.01 * rn(3)
        mp[b] = (cam - pred_t[b]) @ Rs[b]  # R^T (cam - t), so that mp R^T + t = cam
    return Rs.float(), pred_t.float(), mp.float(), target.float()


def drop_point(x, b, i):
    """x [B, P, 3] with point i of crop b replaced by a copy of a point that is not special (index
    1, or 2 when i == 1): as a candidate it is then 'removed' without changing P."""
    out = x.clone()
    out[b, i] = x[b, 1 if i != 1 else 2]
    return out
