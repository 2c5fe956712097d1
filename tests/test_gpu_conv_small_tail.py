"""krrn_conv_small_f32's ragged channel tail (a last tile of one channel quad runs on the 16-block
4x4x1 MFMA where a wave runs at least 8 of the 16-wide K steps, every other remainder as a padded tile;
tiles wholly past N are skipped), called directly over every (nw, ks) and tail shape. "Tail" below is
every channel past the last multiple of 16, whichever form it runs in. K steps = ceil(taps * cin / 16), per
wave ceil(steps / ks): cin 4 / 20 / 36 give 3 / 12 / 21 steps at 3x3 (the 4x4x1 form at ks = 1 for 20, at
ks = 1 and 2 for 36) and 1 - 3 at 1x1 (never); cin 52 gives 30 (8 per wave at ks = 4) and cin 128 gives
72 at 3x3 and 8 at 1x1 (ks = 1), so the 4x4x1 form runs under every ks and for every kind of conv.

Set-up as test_conv_small: NaN-filled output, a guard column block that must stay 0, a channel-offset
input (the columns around it NaN: never read). Small maps, so blocks span rows and images and M is no
multiple of 16.

Numerics rule: the full tiles are an fma chain over k; a tail channel is four per-k-quad chains plus two
adds. Within one test (one reduction length K) the worst error against the f64 result is measured over
every full-tile channel of every launch, and over every tail channel (channels past the last multiple of
16); the tail's may be at most twice the full tiles'. Both must also lie inside the forward error bound
of a length-K f32 sum."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MAPS = [(3, 5, 6), (2, 7, 9), (5, 4, 4)]                # (B, H, W)
COUTS = [4, 8, 12, 18, 20, 24, 36, 40, 44, 72]          # tails of 1, 2, 3 quads after 0, 1, 2, 4 full tiles
CINS = [4, 20, 36, 52, 128]                             # k-quads that do / do not fill the last 16-wide step;
                                                        # 52 and 128: long enough for the 4x4x1 tail at ks = 4 / at 1x1
KINDS = [(3, 1), (3, 2), (1, 1)]                        # (ksize, stride)
CFGS = [(nw, ks) for nw in (1, 2, 3) for ks in (1, 2, 4)]
CO = 4                                                  # input channel offset


def _pad4(c):
    return (c + 3) // 4 * 4


class _Problem:
    """One conv (weights, folded scale / bias, input, residual) on the device, with its f64 results."""

    def __init__(self, dev, B, H, W, cin, cout, k, st, seed):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.B, self.H, self.W, self.cin, self.cout, self.k, self.st = dev, B, H, W, cin, cout, k, st
        self.np_ = np_ = _pad4(cout)
        w = 0.1 * torch.randn(cout, cin, k, k, generator=g)
        x = torch.randn(B, cin, H, W, generator=g)
        scale, bias = torch.zeros(np_), torch.zeros(np_)
        scale[:cout] = 0.7 + 0.6 * torch.rand(cout, generator=g)
        bias[:cout] = 0.1 * torch.randn(cout, generator=g)
        pad = (k - 1) // 2
        y = F.conv2d(x.double(), w.double(), stride=st, padding=pad).permute(0, 2, 3, 1)  # [B, Ho, Wo, cout]
        mag = F.conv2d(x.double().abs(), w.double().abs(), stride=st, padding=pad).permute(0, 2, 3, 1)
        self.Ho, self.Wo = y.shape[1], y.shape[2]
        res = torch.zeros(B, self.Ho, self.Wo, np_)
        res[..., :cout] = torch.randn(B, self.Ho, self.Wo, cout, generator=g)
        s64, b64 = scale[:cout].double(), bias[:cout].double()
        lin = y * s64 + b64
        # {with residual + ReLU: f64 result}, and the forward error bound of the f32 evaluation: a sum of
        # K products and the epilogue's 3 operations, each rounded once (u = 2^-24)
        self.ref = {False: lin.to(dev), True: torch.relu(lin + res[..., :cout].double()).to(dev)}
        K = k * k * cin
        self.bound = {False: ((K + 4) * 2.0 ** -24 * 1.01 * (mag * s64 + b64.abs())).to(dev)}
        self.bound[True] = self.bound[False] + ((K + 4) * 2.0 ** -24 * 1.01 * res[..., :cout].double().abs()).to(dev)
        wt = torch.zeros(np_, k * k, cin)  # [N][tap][cin]; pad rows zero
        wt[:cout] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
        self.cs = cin + CO + 4
        xt = torch.full((B, H, W, self.cs), float("nan"))
        xt[..., CO:CO + cin] = x.permute(0, 2, 3, 1)
        self.xt, self.wt, self.res = xt.to(dev), wt.reshape(np_, -1).contiguous().to(dev), res.to(dev)
        self.scale, self.bias = scale.to(dev), bias.to(dev)

    def run(self, nw, ks, with_res, N=None, images=None):
        """One launch -> the [B, Ho, Wo, np_ + 4] output buffer (N: only the first N weight rows;
        images = (b0, n): a launch over images b0 .. b0 + n - 1 alone)."""
        from pose_estimation_amd import _lib
        from pose_estimation_amd.runtime import P, ptr
        N = self.np_ if N is None else N
        b0, nb = images if images is not None else (0, self.B)
        xt, res = self.xt[b0:b0 + nb], self.res[b0:b0 + nb]
        out = torch.full((nb, self.Ho, self.Wo, self.np_ + 4), float("nan"), device=self.dev)
        out[..., self.np_:] = 0.0
        _lib.check(_lib.lib().krrn_conv_small_f32(
            ptr(xt), self.cs, CO, nb, self.H, self.W, self.cin, ptr(self.wt), N, N, ptr(self.scale), ptr(self.bias),
            ptr(res) if with_res else P(0), self.np_ if with_res else 0, 0, ptr(out), self.np_ + 4, 0,
            int(with_res), self.k, self.st, nw, ks, P(torch.cuda.current_stream().cuda_stream)), "small conv")
        return out


@pytest.mark.parametrize("k,st", KINDS)
@pytest.mark.parametrize("cin", CINS)
def test_tail_error_pads_and_guard(dev, cin, k, st):
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    worst = {"full": zero.clone(), "tail": zero.clone(), "quad": zero.clone()}  # quad: one-quad tails alone
    inside = torch.ones((), dtype=torch.bool, device=dev)   # every error within the forward bound
    clean = torch.ones((), dtype=torch.bool, device=dev)    # pad channels 0.0, guard block 0
    for cout in COUTS:
        nfull = 16 * (cout // 16)  # channels [0, nfull) lie in full tiles, [nfull, cout) in the ragged one
        for mi, (B, H, W) in enumerate(MAPS):
            p = _Problem(dev, B, H, W, cin, cout, k, st, seed=1000 * cin + 10 * cout + 3 * k + st + mi)
            for nw, ks in CFGS:
                for with_res in (False, True):
                    out = p.run(nw, ks, with_res)
                    err = (out[..., :cout].double() - p.ref[with_res]).abs()
                    inside &= (err <= p.bound[with_res]).all()   # NaN (an unwritten channel) fails here
                    if nfull:
                        worst["full"] = torch.maximum(worst["full"], err[..., :nfull].max())
                    worst["tail"] = torch.maximum(worst["tail"], err[..., nfull:].max())
                    if p.np_ % 16 == 4:
                        worst["quad"] = torch.maximum(worst["quad"], err[..., nfull:].max())
                    clean &= (out[..., cout:] == 0.0).all()      # pad channels (18, 19 of 20) and the guard
    full, tail = worst["full"].item(), worst["tail"].item()
    print(f"conv_small cin {cin} {k}x{k}/{st}: worst |err| vs f64, full tiles {full:.3e}, tail {tail:.3e} "
          f"(one-quad tails {worst['quad'].item():.3e})")
    assert clean.item()
    assert inside.item()
    assert full > 0.0 and tail <= 2.0 * full, (full, tail)


@pytest.mark.parametrize("k,st", KINDS)
@pytest.mark.parametrize("cout,nhead", [(36, 32), (72, 64)])
def test_full_tiles_bit_identical_to_launch_without_tail(dev, cout, nhead, k, st):
    """Channels of full tiles equal, bit for bit, a launch over the first nhead weight rows only (N a
    multiple of 16: no tail)."""
    same = torch.ones((), dtype=torch.bool, device=dev)
    for cin in CINS:
        for mi, (B, H, W) in enumerate(MAPS):
            p = _Problem(dev, B, H, W, cin, cout, k, st, seed=77 * cin + cout + 5 * k + st + mi)
            for nw, ks in CFGS:
                for with_res in (False, True):
                    whole = p.run(nw, ks, with_res)
                    head = p.run(nw, ks, with_res, N=nhead)
                    same &= torch.equal(whole[..., :nhead], head[..., :nhead])
                    same &= bool(torch.isnan(head[..., nhead:p.np_]).all())  # the N = nhead launch stops at nhead
    assert same.item()


@pytest.mark.parametrize("k,st", KINDS)
def test_tail_batch_invariance(dev, k, st):
    """The B = 3 result equals, row for row, three B = 1 launches (NaNs included: none are expected)."""
    B, H, W = MAPS[0]
    same = torch.ones((), dtype=torch.bool, device=dev)
    for cin in CINS:
        for cout in COUTS:
            p = _Problem(dev, B, H, W, cin, cout, k, st, seed=31 * cin + 7 * cout + k + st)
            for nw, ks in CFGS:
                whole = p.run(nw, ks, True)
                same &= not bool(torch.isnan(whole[..., :p.np_]).any())
                for b in range(B):
                    same &= torch.equal(whole[b:b + 1], p.run(nw, ks, True, images=(b, 1)))
    assert same.item()
