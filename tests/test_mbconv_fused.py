"""The one-kernel frozen inverted residual (``hip/mbconv_fused.hip``) against
fp64 on the CPU from the bf16 operands, with no intermediate rounding.

Bound, elementwise, derived and not tuned, u = 2^-8, f(n) = (n + 8) 2^-23:
  e1 = u h1 + f(Cin) (|s1| (|x| |w1|^T) + |b1|)
  e2 = u h2 + |s2| dw(e1; |wd|) + f(9) (|s2| dw(h1; |wd|) + |b2|)
  |y - ref| <= u |pre3| + |s3| (e2 |w3|^T) + f(Chid) (|s3| (h2 |w3|^T) + |b3| + |res|)
u is the one rounding to bf16 of h1, h2 and y; f(n) the fp32 recursive-sum
bound over an n-long reduction and the epilogue's few operations, doubled (as
in test_pw_deep.py). ReLU6 is 1-Lipschitz, so each stage's error passes
through it; zero padding applies to e1 as to h1. An fp32/bf16 emulation of the
kernel reaches 0.11-0.25 of the bound; halo pixels left at relu6(b1), a dropped
tap and a dropped hidden tail reach 2.7-46x.
"""
import functools

import pytest
import torch

gpu = pytest.mark.gpu

# (N, H, W, Cin, Chid, Cout, res): one tile with the whole halo outside; 2x2
# tiles with halos from neighbours and a hidden-chunk tail; partial tiles on
# both axes, W below the tile, Cin below one MFMA step; the largest Cin, a
# one-row tile, three tiles across; several chunks plus a tail and the widest
# Cout; a real layer's channels
SHAPES = [(2, 7, 7, 16, 48, 16, True), (1, 14, 14, 24, 72, 40, False),
          (2, 9, 5, 8, 40, 8, True), (1, 8, 15, 160, 104, 24, False),
          (1, 3, 3, 32, 200, 320, False), (1, 15, 8, 96, 576, 96, True)]
_ID = "n%d_%dx%d_c%d_h%d_k%d_res%d"
U = 2.0 ** -8


def _f(n):
    return (n + 8) * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _inputs(N, H, W, Cin, Chid, Cout, seed=0):
    """CPU operands: x [N,H,W,Cin], w1 [Chid,Cin], wd [9,Chid], w3 [Cout,Chid]
    bf16 ~ N(0,1); the three folds put pre1 and pre2 at ~N(3, 3^2)."""
    g = torch.Generator(device="cpu").manual_seed(N * 1000 + H * 100 + W * 10 + Cin + Chid + Cout + seed)
    x, w1, wd, w3 = (torch.randn(*s, generator=g).to(torch.bfloat16)
                     for s in ((N, H, W, Cin), (Chid, Cin), (9, Chid), (Cout, Chid)))

    def uni(c, lo, hi):
        return torch.empty(c).uniform_(lo, hi, generator=g)

    return (x, w1, uni(Chid, .9, 1.1) * 3.0 / Cin ** 0.5, uni(Chid, 2.8, 3.2),
            wd, uni(Chid, .9, 1.1) * 3.0 / 11.0, uni(Chid, 2.8, 3.2),
            w3, uni(Cout, .9, 1.1) / (14.0 * Chid) ** 0.5, uni(Cout, -.5, .5))


def _dw(t, wd):
    """3x3 stride-1 zero-padded depthwise of t [N,H,W,C] with wd [9,C], fp64."""
    H, W = t.shape[1:3]
    p = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
    return sum(p[:, r:r + H, s:s + W] * wd[3 * r + s] for r in range(3) for s in range(3))


def _assert_bound(y, ops, res, what, regions=False):
    """y (device, [N,Cout,H,W]) against the fp64 reference of the CPU operands."""
    x, w1, s1, b1, wd, s2, b2, w3, s3, b3 = (t.double() for t in ops)
    Cin, Chid = x.shape[-1], w1.shape[0]
    pre1 = (x @ w1.t()) * s1 + b1
    h1 = pre1.clamp(0, 6)
    e1 = U * h1 + _f(Cin) * (s1.abs() * (x.abs() @ w1.abs().t()) + b1.abs())
    pre2 = _dw(h1, wd) * s2 + b2
    h2 = pre2.clamp(0, 6)
    e2 = U * h2 + s2.abs() * _dw(e1, wd.abs()) + _f(9) * (s2.abs() * _dw(h1, wd.abs()) + b2.abs())
    r = x if res else torch.zeros(())
    ref = (h2 @ w3.t()) * s3 + b3 + r
    bound = (U * ref.abs() + s3.abs() * (e2 @ w3.abs().t())
             + _f(Chid) * (s3.abs() * (h2 @ w3.abs().t()) + b3.abs() + r.abs()))
    if regions:
        for pre in (pre1, pre2):
            for cnt in ((pre < 0).sum(), ((pre > 0) & (pre < 6)).sum(), (pre > 6).sum()):
                assert cnt.item() / pre.numel() >= 0.05, (what, cnt.item(), pre.numel())
    assert y.dtype == torch.bfloat16 and y.shape == ref.permute(0, 3, 1, 2).shape
    y = y.permute(0, 2, 3, 1).cpu().double()
    assert torch.isfinite(y).all(), what
    worst = ((y - ref).abs() / bound).max().item()
    print(f"{what}: max |y-ref| / bound = {worst:.3f}")
    assert ((y - ref).abs() <= bound).all(), (what, worst)


def _call(ops, res, out=None):
    from ddlw_amd.ops import binding

    dev = torch.device("cuda:0")
    x, *rest = (t.to(dev) for t in ops)
    return binding.mbconv_fused_fwd(x.permute(0, 3, 1, 2), *rest, res, out=out)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[_ID % s for s in SHAPES])
def test_forward(shape):
    ops = _inputs(*shape[:6])
    _assert_bound(_call(ops, shape[6]), ops, shape[6], f"fused {shape}", regions=True)


@gpu
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[_ID % s for s in SHAPES[1:3]])
def test_tails_do_not_leak(shape):
    """Every operand is a slice out of the middle of a NaN buffer, y out of a
    buffer of sentinels: no NaN reaches the result, the sentinels survive."""
    N, H, W, _, _, Cout, res = shape
    ops = _inputs(*shape[:6], seed=1)
    dev, PAD = torch.device("cuda:0"), 64

    def embed(t, fill):
        buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=dev)
        buf[PAD:PAD + t.numel()] = t.to(dev).flatten()
        return buf, buf[PAD:PAD + t.numel()].view(t.shape)

    ybuf, yv = embed(torch.empty(N, H, W, Cout, dtype=torch.bfloat16), -1234.0)
    before = ybuf.clone()
    y = _call([embed(t, float("nan"))[1] for t in ops], res, out=yv.permute(0, 3, 1, 2))
    assert y.data_ptr() == yv.data_ptr()
    _assert_bound(y, ops, res, f"fused tails {shape}")
    assert torch.equal(ybuf[:PAD], before[:PAD]) and torch.equal(ybuf[-PAD:], before[-PAD:])


@gpu
def test_deterministic():
    ops = _inputs(*SHAPES[5][:6])
    assert torch.equal(_call(ops, True), _call(ops, True))


@gpu
@pytest.mark.parametrize("cin,cout,stride,mode,calls",
                         [(24, 24, 1, "1", 1), (64, 96, 1, "1", 1), (24, 24, 1, "0", 0),
                          (64, 96, 1, "0", 0), (24, 32, 2, "1", 0)])
def test_block_route(monkeypatch, cin, cout, stride, mode, calls):
    from ddlw_amd.models.mobilenet_v2 import InvertedResidual
    from ddlw_amd.ops import apply_bf16_policy, binding
    from ddlw_amd.ops.layers import BatchNormAct2d

    torch.manual_seed(cin + cout)
    dev = torch.device("cuda:0")
    blk = apply_bf16_policy(InvertedResidual(cin, cout, stride, 6).to(dev)).eval()
    bns = [m for m in blk.modules() if isinstance(m, BatchNormAct2d)]
    with torch.no_grad():
        for bn in bns:
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(2, 14, 14, cin, device=dev).to(torch.bfloat16)
    seen, real = [], binding.mbconv_fused_fwd
    monkeypatch.setattr(binding, "mbconv_fused_fwd", lambda *a, **k: seen.append(1) or real(*a, **k))
    monkeypatch.setenv("DDLW_MBCONV_FUSED", mode)
    with torch.no_grad():
        y = blk(x.permute(0, 3, 1, 2))
    assert len(seen) == calls
    if calls:
        c1, c2, c3 = blk.conv[0], blk.conv[3], blk.conv[6]
        folds = [t.cpu() for bn in bns for t in bn.folded_scale_bias()]
        ops = (x.cpu(), c1.weight.cpu().reshape(6 * cin, cin), *folds[0:2],
               c2.weight.cpu().reshape(6 * cin, 9).t(), *folds[2:4],
               c3.weight.cpu().reshape(cout, 6 * cin), *folds[4:6])
        _assert_bound(y, ops, blk.use_res, f"block {cin}->{cout}")


def test_supported_and_route(monkeypatch):
    from ddlw_amd.ops import binding

    assert binding.mbconv_fused_supported(160, 960, 320, 1)
    for bad in ((168, 960, 160, 1), (160, 960, 328, 1), (24, 140, 24, 1), (20, 120, 24, 1),
                (24, 144, 36, 1), (24, 144, 24, 2)):
        assert not binding.mbconv_fused_supported(*bad), bad
    shapes = [(c, 6 * c, k, 64 * h * h) for h, c, k in
              ((56, 24, 24), (28, 32, 32), (14, 64, 64), (14, 64, 96), (14, 96, 96),
               (7, 160, 160), (7, 160, 320))]
    monkeypatch.setenv("DDLW_MBCONV_FUSED", "0")
    assert not any(binding.mbconv_fused_route(*s) for s in shapes)
    monkeypatch.setenv("DDLW_MBCONV_FUSED", "1")
    assert all(binding.mbconv_fused_route(*s) for s in shapes)
    assert not binding.mbconv_fused_route(168, 1008, 168, 3136)
    monkeypatch.delenv("DDLW_MBCONV_FUSED")
    for s in shapes:  # unset: exactly the measured winners, inside their row range
        row = binding._MBCONV_FUSED_MEASURED.get(s[:3])
        assert binding.mbconv_fused_route(*s) == (row is not None and row[0] <= s[3] <= row[1])
    assert not binding.mbconv_fused_route(8, 48, 8, 49)  # never measured
