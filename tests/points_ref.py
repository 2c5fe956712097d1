"""Plain CPU references of the point-branch operations of include/krrn_hip.h, one small function per
operation, written from the header comments and the reference model's definitions (gcn3d.py,
fusion.py, posenet.py, krrn.py), not from the kernels. Index / copy / max operations are torch indexing
in f32 (compared bit for bit); arithmetic ones are float64. kNN has two: knn_ref, the pinned f32
expression order of oracle/krrn_oracle.py (exact indices), and knn_check_f64, an independent float64
brute force with a rounding bound that any correct f32 evaluation order meets.

Also here, because the CPU test of the references and the GPU tests share them: the kNN case table with
its input families, and the guarded output buffers (a slice of a wider, sentinel-filled allocation).
"""
import math

import torch
import torch.nn.functional as F

from oracle.krrn_oracle import _seq_sum, _stable_topk_small

EPS32 = 2.0 ** -24  # unit roundoff of f32


# ----------------------------------------------------------------------------------------------
# guarded outputs: [guard row | B x (rows x stride + slack) | guard row], sentinel everywhere
# ----------------------------------------------------------------------------------------------
class Guarded:
    """A [B][rows][width] output slice inside a wider flat allocation filled with a sentinel (NaN for
    floats, -1 for ints): row stride >= width, column offset `off`, batch stride rows * stride + slack,
    one guard row of `stride` elements before and after."""

    def __init__(self, B, rows, width, stride=None, off=0, slack=0, dtype=torch.float32, device="cpu"):
        stride = width if stride is None else stride
        assert off + width <= stride
        self.B, self.rows, self.width, self.stride, self.off = B, rows, width, stride, off
        self.bs = rows * stride + slack
        self.sentinel = float("nan") if dtype.is_floating_point else -1
        self.buf = torch.full((2 * stride + B * self.bs,), self.sentinel, dtype=dtype, device=device)

    @property
    def offset(self):
        """Element offset of slice element (0, 0, 0) in the flat buffer."""
        return self.stride + self.off

    def ptr_value(self):
        return self.buf.data_ptr() + self.offset * self.buf.element_size()

    def _view(self, flat):
        body = flat[self.stride:self.stride + self.B * self.bs].view(self.B, self.bs)
        rows = body[:, :self.rows * self.stride].view(self.B, self.rows, self.stride)  # a view: writes reach `flat`
        return rows[..., self.off:self.off + self.width]

    def fill(self, values):
        """Write `values` [B][rows][width] into the slice (an input that lives in a wider buffer, or an
        output that aliases an input)."""
        self._view(self.buf)[...] = values.to(self.buf.device)

    def result(self):
        """(slice [B][rows][width] on the CPU) after asserting that the slice holds no sentinel and that
        every element outside it still holds the sentinel's bit pattern."""
        flat = self.buf.cpu()
        got = self._view(flat).clone(memory_format=torch.contiguous_format)
        bits = flat.view(torch.int32) if flat.element_size() == 4 else flat.view(torch.int64)
        sent = torch.full((1,), self.sentinel, dtype=flat.dtype)
        sent = int((sent.view(torch.int32) if flat.element_size() == 4 else sent.view(torch.int64))[0])
        outside = torch.ones_like(bits, dtype=torch.bool)
        self._view(outside)[...] = False
        assert int(outside.sum()) == flat.numel() - self.B * self.rows * self.width
        touched = (bits != sent) & outside
        assert not touched.any(), f"{int(touched.sum())} elements outside the slice were written, first at " \
                                  f"{int(touched.nonzero()[0])} (slice starts at {self.offset})"
        if flat.dtype.is_floating_point:
            assert not torch.isnan(got).any(), "sentinel (NaN) left inside the slice"
        else:
            assert (got != self.sentinel).all(), "sentinel (-1) left inside the slice"
        return got


# ----------------------------------------------------------------------------------------------
# index, copy and max operations (f32, bit-exact)
# ----------------------------------------------------------------------------------------------
def _bi(B):
    return torch.arange(B)[:, None, None]


def pool_max_ref(Fm, nbr):
    """out[b, t, :] = max_j F[b, nbr[b, t, j], :] (gcn3d.py:233-236). F [B][n][C], nbr [B][nq][kk]."""
    return Fm[_bi(Fm.shape[0]), nbr.long()].max(dim=2).values


def gather_rows_ref(src, idx, B):
    """dst[b, r, :] = src[b, idx[b, r], :]; src [B or 1][n][w] and idx [B or 1][nrows] (a leading 1 = the
    batch shares it: src_bs = 0 / idx_bs = 0)."""
    src = src.expand(B, -1, -1)
    idx = idx.expand(B, -1).long()
    return src[torch.arange(B)[:, None], idx]


def points_gather_ref(cloud, xyz, nml, choose):
    """P9 [B][N][9] = [cloud | xyz at choose | nml at choose] (krrn.py:121-122, fusion.py:194)."""
    B = cloud.shape[0]
    ch = choose.view(B, 1, -1).repeat(1, 3, 1)
    xe = torch.gather(xyz.reshape(B, 3, -1), -1, ch).permute(0, 2, 1)
    ne = torch.gather(nml.reshape(B, 3, -1), -1, ch).permute(0, 2, 1)
    return torch.cat([cloud, xe, ne], 2)


def nchw_to_nhwc_ref(x):
    return x.permute(0, 2, 3, 1).contiguous()


def add_relu_ref(a, b, relu):
    r = a if b is None else a + b
    return torch.relu(r) if relu else r.clone()


def heads_select_ref(fx, xyz_off, fn, cls):
    """(xyz f32 exact, normal float64): the crop's class block of the xyz / normal maps and
    F.normalize(p=2, dim=1, eps=1e-12) = x / max(||x||, 1e-12) (krrn.py:105-108)."""
    B = fx.shape[0]
    xyz = torch.stack([fx[b, xyz_off + 3 * int(cls[b]):xyz_off + 3 * int(cls[b]) + 3] for b in range(B)])
    n = torch.stack([fn[b, 3 * int(cls[b]):3 * int(cls[b]) + 3] for b in range(B)]).double()
    return xyz, n / n.norm(dim=1, keepdim=True).clamp_min(1e-12)


# ----------------------------------------------------------------------------------------------
# arithmetic operations (float64)
# ----------------------------------------------------------------------------------------------
def gather2_add_ref(ia, A, ib, Bm, scale, bias, bias2, relu):
    """(out, bound), float64: out[b, i] = act(scale * (A[b, ia[b, i]] + B[b, ib[b, i]]) + bias + bias2[b]);
    bound = 4 * 2^-24 * (|scale| (|A| + |B|) + |bias| + |bias2|): at most four roundings, contracted or
    not."""
    B = A.shape[0]
    bi = torch.arange(B)[:, None]
    a, b = A.double()[bi, ia.long()], Bm.double()[bi, ib.long()]
    s, c = scale.double(), bias.double()
    c2 = bias2.double()[:, None, :] if bias2 is not None else torch.zeros(B, 1, A.shape[-1], dtype=torch.float64)
    out = s * (a + b) + c + c2
    bound = 4 * EPS32 * (s.abs() * (a.abs() + b.abs()) + c.abs() + c2.abs())
    return (torch.relu(out) if relu else out), bound


def tbase_tail_ref(h, w4, b4, cloud):
    """(t_res, pred_t, t_bound, p_bound), float64: t_res[b, i] = W4 h[b, i] + b4 (posenet.py:76-80, the first
    three outputs), pred_t[b] = mean_i(cloud[b, i] + t_res[b, i]) (krrn.py:153).
    t_bound = (C + 1) 2^-24 (sum_c |w h| + |b|); p_bound = mean_i t_bound + m 2^-24 mean_i(|cloud| + |t|),
    m = ceil(n / 256) + 4 + 16 + 2: a lane's serial passes, four shuffle levels, the 16-wave loop, the
    add and the divide of the documented summation order."""
    n, C = h.shape[1], h.shape[2]
    h64, w64, b64, c64 = h.double(), w4.double(), b4.double(), cloud.double()
    t = h64 @ w64.t() + b64
    t_bound = (C + 1) * EPS32 * (h64.abs() @ w64.abs().t() + b64.abs())
    pred = (c64 + t).mean(dim=1)
    m = math.ceil(n / 256) + 4 + 16 + 2
    p_bound = t_bound.mean(dim=1) + m * EPS32 * (c64.abs() + t.abs()).mean(dim=1)
    return t, pred, t_bound, p_bound


def resize_ref(x, Ho, Wo, align):
    """F.interpolate(mode='bilinear') of an NCHW map in float64."""
    return F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=align)


# ----------------------------------------------------------------------------------------------
# kNN
# ----------------------------------------------------------------------------------------------
def knn_ref(q, c, k, drop_first=0, mode=0, qidx=None):
    """Reference (a): the oracle's pinned f32 expression order (_seq_sum over the coordinates, every
    operation rounded) and tie rule (stable sort: the lower index wins), for separate query and candidate
    sets. q [B][n][d] (rows qidx if given), c [B or 1][nc][d];
      mode 0 (get_neighbor_index, gcn3d.py:23): ((-2 <q,c>) + |c|^2) + |q|^2
      mode 1 (get_nearest_index, gcn3d.py:36):  (|c|^2 + |q|^2) - 2 <q,c>
    Returns int64 [B][nq][k]: the k + drop_first nearest without the first drop_first."""
    if qidx is not None:
        q = q[:, qidx.long()]
    inner = _seq_sum(q[:, :, None, :] * c[:, None, :, :])
    cn, qn = _seq_sum(c * c), _seq_sum(q * q)
    if mode == 0:
        dist = (inner * -2.0 + cn[:, None, :]) + qn[:, :, None]
    else:
        dist = (cn[:, None, :] + qn[:, :, None]) - 2.0 * inner
    return _stable_topk_small(dist, k + drop_first)[..., drop_first:]


def knn_check_f64(q, c, idx, K):
    """Check (b) on the K indices idx [B][nq][K] returned for queries q [B][nq][d] among c [B or 1][nc][d]
    (nothing dropped): every index in [0, nc), no repeats in a row, and with D64 the float64 squared
    distances and e = (d + 2) 2^-24 2 (|q|^2 + max_j |c_j|^2) (the rounding of the three sequential sums
    and the two combining operations): max over the returned D64 <= K-th smallest D64 + 2 e.
    Returns the largest used fraction of the slack 2 e (0 where the K-th distance is met exactly)."""
    d, nc = q.shape[-1], c.shape[1]
    idx = idx.long()
    assert idx.shape[-1] == K
    assert (idx >= 0).all() and (idx < nc).all(), "index outside [0, nc)"
    srt = idx.sort(dim=-1).values
    assert (srt[..., 1:] != srt[..., :-1]).all(), "a row repeats an index"
    q64, c64 = q.double(), c.double()
    D = ((q64[:, :, None, :] - c64[:, None, :, :]) ** 2).sum(-1)          # [B][nq][nc]
    e = (d + 2) * EPS32 * 2 * ((q64 ** 2).sum(-1) + (c64 ** 2).sum(-1).max(dim=1).values[:, None])
    kth = D.sort(dim=-1).values[..., K - 1]
    worst = torch.gather(D, -1, idx).max(dim=-1).values
    over = worst - kth
    assert (over <= 2 * e).all(), f"a returned neighbour is {float((over / (2 * e).clamp_min(1e-300)).max()):.3g} x the " \
                                  "rounding slack beyond the K-th nearest"
    return float((over / (2 * e).clamp_min(1e-300)).max())


def knn_points(family, B, n, d, g):
    """The input families of the kNN tests, [B][n][d] f32 from the seeded generator g."""
    if family == "random":
        return torch.randn(B, n, d, generator=g)
    if family == "lattice":  # small integer coordinates: many exact distance ties
        return torch.randint(0, 4, (B, n, d), generator=g).float()
    if family == "cloud":  # a depth crop: ~0.1 m extent around (0.02, -0.05, 0.9), where the f32
        # cancellation in |c|^2 + |q|^2 - 2 <q,c> is worst; the 9-D rows add normalised xyz and unit normals
        v = torch.tensor([0.02, -0.05, 0.9]) + 0.1 * (torch.rand(B, n, 3, generator=g) - 0.5)
        if d == 9:
            nm = torch.randn(B, n, 3, generator=g)
            v = torch.cat([v, torch.rand(B, n, 3, generator=g), nm / nm.norm(dim=-1, keepdim=True)], 2)
        return v.contiguous()
    if family == "dup":  # two duplicated points
        v = torch.randn(B, n, d, generator=g)
        v[:, n - 1] = v[:, 0]
        if n > 3:
            v[:, n // 2] = v[:, 1]
        return v
    if family == "same":  # every point identical: the answer is drop .. K - 1 ascending
        return torch.randn(1, 1, d, generator=g).expand(B, n, d).contiguous()
    raise ValueError(family)


# (id, d, B, nq, nc, k, drop_first, mode, family, layout). K = k + drop_first picks the kept-list size
# KS in {1, 2, 5, 8, 11, 16}; the lanes-per-query form is 16 iff cdiv(nq, 64) * B < 1024 and nc >= 768,
# else 4; a second LDS chunk needs nc > 1024. layout: "dense" = contiguous rows, per-crop candidates;
# "shared" = one candidate set for the batch (c_bs = 0); "strided" = d = 3 rows of a [B][n][9] buffer
# (q_st = c_st = 9, batch stride with slack), queries = a shuffled subset qidx shared by the batch, the
# candidates all n = nc rows.
KNN_CASES = [
    # ---- 4 lanes per query: nc in {K, K + 1, 5, 63, 767}; nq in {1, 65, 77}
    ("l4-d3-KS1-K1-nc=K-sentinels", 3, 2, 1, 1, 1, 0, 1, "random", "dense"),
    ("l4-d3-KS2-K2-nc=K+1", 3, 2, 65, 3, 1, 1, 0, "cloud", "dense"),
    ("l4-d3-KS5-K3-nc5-sentinels", 3, 2, 77, 5, 2, 1, 0, "lattice", "dense"),
    ("l4-d3-KS5-K5-nc=K-sentinels", 3, 3, 65, 5, 5, 0, 1, "random", "dense"),
    ("l4-d3-KS8-K6-nc63", 3, 2, 77, 63, 5, 1, 0, "cloud", "dense"),
    ("l4-d3-KS8-K8-nc=K+1", 3, 2, 1, 9, 8, 0, 0, "dup", "dense"),
    ("l4-d3-KS11-K9-nc767", 3, 2, 65, 767, 8, 1, 0, "lattice", "dense"),
    ("l4-d3-KS11-K11-nc767-cloud", 3, 2, 77, 767, 10, 1, 0, "cloud", "dense"),
    ("l4-d3-KS16-K12-nc=K-sentinels", 3, 2, 65, 12, 12, 0, 1, "random", "dense"),
    ("l4-d3-KS16-K16-nc=K+1", 3, 2, 77, 17, 15, 1, 0, "dup", "dense"),
    ("l4-d3-KS16-K16-nc=K-same", 3, 2, 65, 16, 16, 0, 0, "same", "dense"),
    ("l4-d9-KS1-K1-nc5", 9, 2, 65, 5, 1, 0, 1, "cloud", "dense"),
    ("l4-d9-KS2-K2-nc=K-sentinels", 9, 2, 1, 2, 1, 1, 0, "random", "dense"),
    ("l4-d9-KS5-K5-nc=K+1", 9, 2, 77, 6, 4, 1, 0, "lattice", "dense"),
    ("l4-d9-KS5-K3-nc63", 9, 2, 65, 63, 3, 0, 1, "dup", "dense"),
    ("l4-d9-KS8-K8-nc767", 9, 2, 77, 767, 7, 1, 0, "cloud", "dense"),
    ("l4-d9-KS8-K6-nc=K-sentinels", 9, 2, 65, 6, 6, 0, 0, "random", "dense"),
    ("l4-d9-KS11-K11-nc=K+1", 9, 2, 1, 12, 10, 1, 0, "random", "dense"),
    ("l4-d9-KS11-K9-nc63-same", 9, 2, 77, 63, 8, 1, 1, "same", "dense"),
    ("l4-d9-KS16-K12-nc767", 9, 2, 65, 767, 11, 1, 0, "lattice", "dense"),
    ("l4-d9-KS16-K16-nc=K-sentinels", 9, 2, 77, 16, 16, 0, 1, "cloud", "dense"),
    # ---- 16 lanes per query: nc in {768, 1000, 1024, 1025, 2049}; nq in {1, 17, 250}
    ("l16-d3-KS1-K1-nc768-nearest", 3, 2, 250, 768, 1, 0, 1, "cloud", "dense"),
    ("l16-d3-KS2-K2-nc1000", 3, 2, 17, 1000, 1, 1, 0, "lattice", "dense"),
    ("l16-d3-KS5-K5-nc1024-pool", 3, 2, 250, 1024, 4, 1, 0, "cloud", "dense"),
    ("l16-d3-KS5-K3-nc1025-chunk2", 3, 2, 1, 1025, 3, 0, 1, "random", "dense"),
    ("l16-d3-KS8-K8-nc1025-chunk2", 3, 2, 17, 1025, 7, 1, 0, "dup", "dense"),
    ("l16-d3-KS8-K6-nc2049-chunk3", 3, 2, 17, 2049, 6, 0, 0, "lattice", "dense"),
    ("l16-d3-KS11-K11-nc2049-chunk3", 3, 2, 250, 2049, 10, 1, 0, "cloud", "dense"),
    ("l16-d3-KS11-K9-nc1000-same", 3, 2, 17, 1000, 9, 0, 1, "same", "dense"),
    ("l16-d3-KS16-K16-nc1025-chunk2", 3, 2, 17, 1025, 15, 1, 0, "random", "dense"),
    ("l16-d3-KS16-K12-nc768", 3, 2, 1, 768, 12, 0, 0, "cloud", "dense"),
    ("l16-d9-KS1-K1-nc1025-chunk2", 9, 2, 17, 1025, 1, 0, 1, "cloud", "dense"),
    ("l16-d9-KS2-K2-nc768", 9, 2, 250, 768, 2, 0, 0, "lattice", "dense"),
    ("l16-d9-KS5-K5-nc2049-chunk3", 9, 2, 17, 2049, 4, 1, 0, "cloud", "dense"),
    ("l16-d9-KS5-K3-nc1000", 9, 2, 1, 1000, 2, 1, 0, "dup", "dense"),
    ("l16-d9-KS8-K8-nc1024", 9, 2, 250, 1024, 8, 0, 1, "random", "dense"),
    ("l16-d9-KS8-K6-nc1025-chunk2", 9, 2, 17, 1025, 5, 1, 0, "same", "dense"),
    ("l16-d9-KS11-K11-nc1000", 9, 2, 17, 1000, 10, 1, 0, "cloud", "dense"),
    ("l16-d9-KS11-K9-nc2049-chunk3", 9, 2, 1, 2049, 9, 0, 1, "lattice", "dense"),
    ("l16-d9-KS16-K16-nc768", 9, 2, 17, 768, 16, 0, 0, "cloud", "dense"),
    ("l16-d9-KS16-K12-nc1025-chunk2", 9, 2, 250, 1025, 11, 1, 0, "random", "dense"),
    # ---- 4 lanes across a chunk edge: cdiv(nq, 64) * B >= 1024 with nc > 1024; one shared candidate set
    # (c_bs = 0), per-crop queries: the production level-0 nearest search for N = 4096, B >= 16
    ("l4-d3-KS1-K1-nc1025-chunk2-shared-c_bs0", 3, 1024, 3, 1025, 1, 0, 1, "cloud", "shared"),
    ("l4-d9-KS11-K11-nc1025-chunk2-shared-c_bs0", 9, 1024, 3, 1025, 10, 1, 0, "random", "shared"),
    # ---- qidx + strided rows of a [B][n][9] buffer, d = 3
    ("l4-d3-KS5-K5-nc300-qidx-strided9", 3, 3, 75, 300, 4, 1, 0, "cloud", "strided"),
    ("l16-d3-KS5-K5-nc1000-qidx-strided9-pool", 3, 2, 250, 1000, 4, 1, 0, "cloud", "strided"),
    ("l16-d3-KS11-K11-nc1030-qidx-strided9-chunk2-lattice", 3, 2, 65, 1030, 10, 1, 0, "lattice", "strided"),
]


def knn_lanes(B, nq, nc):
    """Lanes per query krrn_knn_f32 dispatches (gcn.hip): 16 iff 4 would leave under 1024 blocks and
    every lane still scans >= 48 candidates."""
    return 16 if ((nq + 63) // 64) * B < 1024 and nc >= 768 else 4


def knn_case_inputs(case):
    """(buf, qidx, q, c) of a KNN_CASES row: `buf` the [B][n][w] f32 buffer the rows live in (None unless
    strided), qidx the shared int32 query subset (or None), q [B][nq][d] the queries after qidx and c
    [B or 1][nc][d] the candidates as dense tensors for the references."""
    name, d, B, nq, nc, k, drop, mode, family, layout = case
    g = torch.Generator().manual_seed(1000 * d + 7 * nc + 13 * nq + k + 31 * B)
    if layout == "strided":
        v = knn_points(family, B, nc, 9, g)
        qidx = torch.randperm(nc, generator=g)[:nq].int()
        c = v[..., :3].contiguous()
        return v, qidx, c[:, qidx.long()], c
    if layout == "shared":
        c = knn_points(family, 1, nc, d, g)
        q = knn_points(family, B, nq, d, g)
        if family != "same":
            q[::2] = c[0, :nq]  # every other crop queries candidates themselves (distance 0 at one index)
        return None, None, q, c
    c = knn_points(family, B, nc, d, g)
    if family == "same":
        q = c[:, :1].expand(B, nq, d).contiguous()
    elif nq <= nc:
        q = c[:, :nq].clone()  # self-search on the first nq rows: drop_first drops the point itself
    else:
        q = torch.cat([c, knn_points(family, B, nq - nc, d, g)], 1)
    return None, None, q, c
