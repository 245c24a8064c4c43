"""The stride-2 block kernel (``k_mbconv_fused_s2``) and the ``t = 1`` block
kernel (``k_dwpw_fused``) of ``hip/mbconv_fused.hip`` against fp64 on the CPU
from the bf16 operands, with no intermediate rounding.

The bound is the one derived in ``test_mbconv_fused.py`` (u = 2^-8,
f(n) = (n + 8) 2^-23), elementwise, with dw taken at the block's stride:
  e1 = u h1 + f(Cin) (|s1| (|x| |w1|^T) + |b1|)      (t = 1: h1 = x, e1 = 0)
  e2 = u h2 + |s2| dw(e1; |wd|) + f(9) (|s2| dw(h1; |wd|) + |b2|)
  |y - ref| <= u |ref| + |s3| (e2 |w3|^T) + f(Chid) (|s3| (h2 |w3|^T) + |b3| + |res|)
"""
import functools

import pytest
import torch
from test_mbconv_fused import U, _f, _inputs

gpu = pytest.mark.gpu

# (N, H, W, Cin, Chid, Cout): one exact tile, even size (top / left pad only),
# Cin below an MFMA step, a chunk plus a 32-channel tail; odd H and W (bottom /
# right pad read), partial tile on Y, an 8-channel tail; below one tile; 2x3
# tiles, partial on X, several chunks plus a tail, the TH = 7 LDS maximum;
# TH = 4 with two tiles of 4 + 3 rows, NPW = 2; the widest Cout, NPW = 3
S2_SHAPES = [(2, 14, 14, 16, 96, 24), (1, 15, 13, 24, 72, 32), (2, 9, 5, 8, 40, 8),
             (1, 28, 30, 32, 200, 64), (1, 14, 14, 96, 576, 160), (1, 3, 3, 96, 104, 320)]
# (N, H, W, C, Cout, res)
T1_SHAPES = [(2, 14, 14, 32, 16, False), (1, 15, 9, 32, 16, False), (2, 9, 5, 8, 8, True),
             (1, 30, 17, 40, 24, False), (1, 3, 3, 64, 64, True)]


def _ids(shapes):
    return ["x".join(str(int(v)) for v in s) for s in shapes]


@functools.lru_cache(maxsize=None)
def _t1_inputs(N, H, W, C, Cout, seed=0):
    """CPU operands of the t = 1 block: x [N,H,W,C], wd [9,C], w3 [Cout,C] bf16
    ~ N(0,1); pre2 ~ N(3, 3^2)."""
    g = torch.Generator(device="cpu").manual_seed(N * 1000 + H * 100 + W * 10 + C + Cout + seed)
    x, wd, w3 = (torch.randn(*s, generator=g).to(torch.bfloat16)
                 for s in ((N, H, W, C), (9, C), (Cout, C)))

    def uni(c, lo, hi):
        return torch.empty(c).uniform_(lo, hi, generator=g)

    return (x, wd, uni(C, .9, 1.1), uni(C, 2.8, 3.2),
            w3, uni(Cout, .9, 1.1) / (14.0 * C) ** 0.5, uni(Cout, -.5, .5))


def _dw(t, wd, stride):
    """3x3 pad-1 depthwise of t [N,H,W,C] with wd [9,C] at ``stride``, fp64."""
    H, W = t.shape[1:3]
    p = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
    full = sum(p[:, r:r + H, s:s + W] * wd[3 * r + s] for r in range(3) for s in range(3))
    return full[:, ::stride, ::stride]


def _assert_bound(y, ops, stride, res, what, regions=False):
    """y (device, [N,Cout,Ho,Wo]) against the fp64 reference of the CPU
    operands: ten of them for an expanded block, seven for the t = 1 block."""
    ops = [t.double() for t in ops]
    x, pres = ops[0], []
    if len(ops) == 10:
        w1, s1, b1 = ops[1:4]
        pres.append((x @ w1.t()) * s1 + b1)
        h1 = pres[0].clamp(0, 6)
        e1 = U * h1 + _f(x.shape[-1]) * (s1.abs() * (x.abs() @ w1.abs().t()) + b1.abs())
    else:
        h1, e1 = x, torch.zeros_like(x)
    wd, s2, b2, w3, s3, b3 = ops[-6:]
    pres.append(_dw(h1, wd, stride) * s2 + b2)
    h2 = pres[-1].clamp(0, 6)
    e2 = (U * h2 + s2.abs() * _dw(e1, wd.abs(), stride)
          + _f(9) * (s2.abs() * _dw(h1.abs(), wd.abs(), stride) + b2.abs()))
    r = x if res else torch.zeros(())
    ref = (h2 @ w3.t()) * s3 + b3 + r
    bound = (U * ref.abs() + s3.abs() * (e2 @ w3.abs().t())
             + _f(w3.shape[1]) * (s3.abs() * (h2 @ w3.abs().t()) + b3.abs() + r.abs()))
    if regions:
        for pre in pres:
            for cnt in ((pre < 0).sum(), ((pre > 0) & (pre < 6)).sum(), (pre > 6).sum()):
                assert cnt.item() / pre.numel() >= 0.05, (what, cnt.item(), pre.numel())
    assert y.dtype == torch.bfloat16 and y.shape == ref.permute(0, 3, 1, 2).shape
    y = y.permute(0, 2, 3, 1).cpu().double()
    assert torch.isfinite(y).all(), what
    worst = ((y - ref).abs() / bound).max().item()
    print(f"{what}: max |y-ref| / bound = {worst:.3f}")
    assert ((y - ref).abs() <= bound).all(), (what, worst)


def _call(ops, res=False, out=None):
    """The stride-2 kernel for ten operands, the t = 1 kernel for seven."""
    from ddlw_amd.ops import binding

    x, *rest = (t.to("cuda:0") for t in ops)
    if len(ops) == 10:
        return binding.mbconv_fused_s2_fwd(x.permute(0, 3, 1, 2), *rest, out=out)
    return binding.dwpw_fused_fwd(x.permute(0, 3, 1, 2), *rest, res, out=out)


@gpu
@pytest.mark.parametrize("shape", S2_SHAPES, ids=_ids(S2_SHAPES))
def test_s2_forward(shape):
    ops = _inputs(*shape)
    _assert_bound(_call(ops), ops, 2, False, f"s2 {shape}", regions=True)


@gpu
@pytest.mark.parametrize("shape", T1_SHAPES, ids=_ids(T1_SHAPES))
def test_t1_forward(shape):
    ops = _t1_inputs(*shape[:5])
    _assert_bound(_call(ops, shape[5]), ops, 1, shape[5], f"t1 {shape}", regions=True)


@gpu
@pytest.mark.parametrize("shape", [S2_SHAPES[1], T1_SHAPES[2]], ids=["s2", "t1"])
def test_tails_do_not_leak(shape):
    """Every operand is a slice out of the middle of a NaN buffer, y out of a
    buffer of sentinels: no NaN reaches the result, the sentinels survive."""
    s2 = len(shape) == 6 and not isinstance(shape[5], bool)
    ops = _inputs(*shape, seed=1) if s2 else _t1_inputs(*shape[:5], seed=1)
    N, H, W = shape[:3]
    stride, res, Cout = (2, False, shape[5]) if s2 else (1, shape[5], shape[4])
    dev, PAD = torch.device("cuda:0"), 64

    def embed(t, fill):
        buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=dev)
        buf[PAD:PAD + t.numel()] = t.to(dev).flatten()
        return buf, buf[PAD:PAD + t.numel()].view(t.shape)

    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    ybuf, yv = embed(torch.empty(N, Ho, Wo, Cout, dtype=torch.bfloat16), -1234.0)
    before = ybuf.clone()
    y = _call([embed(t, float("nan"))[1] for t in ops], res, out=yv.permute(0, 3, 1, 2))
    assert y.data_ptr() == yv.data_ptr()
    _assert_bound(y, ops, stride, res, f"tails {shape}")
    assert torch.equal(ybuf[:PAD], before[:PAD]) and torch.equal(ybuf[-PAD:], before[-PAD:])


@gpu
@pytest.mark.parametrize("kind", ["s2", "t1"])
def test_deterministic(kind):
    ops = _inputs(*S2_SHAPES[4]) if kind == "s2" else _t1_inputs(*T1_SHAPES[4][:5])
    assert torch.equal(_call(ops, kind == "t1"), _call(ops, kind == "t1"))


@gpu
@pytest.mark.parametrize("mode", ["1", "0", None])
@pytest.mark.parametrize("cfg,switch,name", [((16, 24, 2, 6), "DDLW_MBCONV_S2", "mbconv_fused_s2_fwd"),
                                             ((32, 16, 1, 1), "DDLW_MBCONV_T1", "dwpw_fused_fwd")],
                         ids=["s2", "t1"])
def test_block_route(monkeypatch, cfg, switch, name, mode):
    from ddlw_amd.models.mobilenet_v2 import InvertedResidual
    from ddlw_amd.ops import apply_bf16_policy, binding
    from ddlw_amd.ops.layers import BatchNormAct2d

    cin, cout, stride, t = cfg
    torch.manual_seed(cin + cout)
    dev = torch.device("cuda:0")
    blk = apply_bf16_policy(InvertedResidual(*cfg).to(dev)).eval()
    bns = [m for m in blk.modules() if isinstance(m, BatchNormAct2d)]
    with torch.no_grad():
        for bn in bns:
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(2, 14, 14, cin, device=dev).to(torch.bfloat16)
    calls = {n: 0 for n in (name, "pw_conv_fwd", "depthwise_fwd_ep")}
    for n in calls:
        monkeypatch.setattr(binding, n, lambda *a, _n=n, _real=getattr(binding, n), **k:
                            calls.__setitem__(_n, calls[_n] + 1) or _real(*a, **k))
    if mode is None:
        monkeypatch.delenv(switch, raising=False)
    else:
        monkeypatch.setenv(switch, mode)
    with torch.no_grad():
        y = blk(x.permute(0, 3, 1, 2))
    if mode != "1":
        assert calls == {name: 0, "pw_conv_fwd": 1 if t == 1 else 2, "depthwise_fwd_ep": 1}
        return
    assert calls == {name: 1, "pw_conv_fwd": 0, "depthwise_fwd_ep": 0}
    convs = [m for m in blk.conv if isinstance(m, torch.nn.Conv2d)]
    ops = [x.cpu()]
    for conv, bn in zip(convs, bns):
        w = conv.weight.cpu()
        ops += [w.reshape(w.shape[0], 9).t() if conv.groups > 1 else w.reshape(w.shape[:2]),
                *(f.cpu() for f in bn.folded_scale_bias())]
    _assert_bound(y, ops, stride, blk.use_res, f"block {cfg}")


def test_supported_and_route(monkeypatch):
    from ddlw_amd.ops import binding as b

    assert b.mbconv_fused_s2_supported(96, 576, 320) and b.dwpw_fused_supported(64, 64)
    for bad in ((104, 624, 160), (96, 576, 328), (24, 140, 32), (20, 120, 24), (24, 144, 36)):
        assert not b.mbconv_fused_s2_supported(*bad), bad
    for bad in ((72, 16), (32, 72), (12, 16), (32, 20), (0, 16)):
        assert not b.dwpw_fused_supported(*bad), bad
    for switch, route, table, shapes in (
            ("DDLW_MBCONV_S2", b.mbconv_fused_s2_route, b._MBCONV_S2_MEASURED,
             [(c, 6 * c, k, 64 * h * h) for h, c, k in ((56, 16, 24), (28, 24, 32), (14, 32, 64), (7, 96, 160))]),
            ("DDLW_MBCONV_T1", b.dwpw_fused_route, b._DWPW_MEASURED, [(32, 16, 64 * 112 * 112)])):
        monkeypatch.setenv(switch, "0")
        assert not any(route(*s) for s in shapes)
        monkeypatch.setenv(switch, "1")
        assert all(route(*s) for s in shapes)
        assert not route(*(104,) * (len(shapes[0]) - 1), 3136)  # unsupported
        monkeypatch.delenv(switch)
        for s in shapes:  # unset: exactly the measured winners, inside their row range
            row = table.get(s[:-1])
            assert route(*s) == (row is not None and row[0] <= s[-1] <= row[1])
            assert not route(*s[:-1], 98)  # below every measured range
        assert not route(*(8,) * (len(shapes[0]) - 1), 49)  # never measured
