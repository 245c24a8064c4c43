"""Depthwise 3x3 backward kernels (dgrad, wgrad) vs the fp32 stock gradients
on the same bf16-rounded inputs, and the Conv2d route that uses them.

Bound: max|err| / max|ref| < 5e-2, the bound tests/test_conv_kernels.py uses
for every conv direction. Shapes are the smallest that reach each way the
kernels can go wrong (see the table in SHAPES).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 5e-2

# (N, H, W, C, stride), pad 1, 3x3
SHAPES = [
    (3, 20, 20, 96, 1),   # the forward test's own shape
    (3, 20, 20, 96, 2),   # ... stride 2
    (2, 15, 15, 24, 2),   # odd spatial + stride 2; vecC = 3 (no power of two)
    (2, 15, 17, 24, 1),   # non-square
    (2, 7, 7, 576, 2),    # Ho = 4
    (1, 2, 2, 960, 1),    # last-stage shape at 64x64 input: every tap pads
    (1, 1, 1, 8, 1),      # single vector, single pixel
    (4, 28, 28, 32, 1),   # 3136 rows: many wgrad row-slice partials
    (1, 3, 3, 2056, 1),   # vecC = 257: a second, partly idle wgrad block column
]
ODD_S2 = (2, 15, 15, 24, 2)


def _cuda():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _out_hw(h, w, st):
    return (h + 2 - 3) // st + 1, (w + 2 - 3) // st + 1


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs + fp32 reference gradients, computed once per shape and shared
    (never modified) by the tests below."""
    n, h, w, c, st = shape
    g = torch.Generator(device="cpu").manual_seed(1000 + sum(shape))
    ho, wo = _out_hw(h, w, st)
    x = _cl(torch.randn(n, c, h, w, generator=g).to(_cuda()).to(torch.bfloat16))
    wt = torch.randn(c, 1, 3, 3, generator=g).to(_cuda()).to(torch.bfloat16)
    dy = _cl(torch.randn(n, c, ho, wo, generator=g).to(_cuda()).to(torch.bfloat16))
    ref_dx = torch.nn.grad.conv2d_input(
        (n, c, h, w), wt.float(), dy.float(), stride=st, padding=1, groups=c)
    ref_dw = torch.nn.grad.conv2d_weight(
        x.float(), (c, 1, 3, 3), dy.float(), stride=st, padding=1, groups=c)
    return x, wt, dy, ref_dx, ref_dw


def _rel(got, ref):
    return ((got.float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()


@pytest.mark.parametrize("shape", SHAPES)
def test_depthwise_dgrad_parity(shape):
    from ddlw_amd.ops import binding

    x, wt, dy, ref_dx, _ = _case(shape)
    dx = binding.depthwise_dgrad(dy, wt, tuple(x.shape), shape[4], 1)
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    err = _rel(dx, ref_dx)
    print(f"dgrad {shape}: rel err {err:.3e}")
    assert err < BOUND, (shape, err)
    dx2 = binding.depthwise_dgrad(dy, wt, tuple(x.shape), shape[4], 1)
    assert torch.equal(dx, dx2), "dgrad not bit-reproducible"


@pytest.mark.parametrize("shape", SHAPES)
def test_depthwise_wgrad_parity(shape):
    from ddlw_amd.ops import binding

    x, wt, dy, _, ref_dw = _case(shape)
    dw = binding.depthwise_wgrad(dy, x, tuple(wt.shape), shape[4], 1)
    assert dw.shape == wt.shape
    err = _rel(dw, ref_dw)
    print(f"wgrad {shape}: rel err {err:.3e}")
    assert err < BOUND, (shape, err)
    dw2 = binding.depthwise_wgrad(dy, x, tuple(wt.shape), shape[4], 1)
    assert torch.equal(dw, dw2), "wgrad not bit-reproducible"


def test_depthwise_wgrad_uses_many_partials():
    """The 3136-row shape must really exercise the cross-block reduction."""
    from ddlw_amd.ops import binding

    n, h, w, c, st = (4, 28, 28, 32, 1)
    assert binding._depthwise_wgrad_nparts(n * h * w, c) > 8


def test_depthwise_dgrad_writes_every_pixel():
    """Stride 2 with odd H/W leaves dx pixels that no tap reaches; they must
    still be written (zero), not left as whatever the allocation held."""
    from ddlw_amd.ops import binding

    n, h, w, c, st = ODD_S2
    x, wt, dy, _, _ = _case(ODD_S2)
    # put non-zero bytes into the block the caching allocator will hand out
    junk = torch.full((n, c, h, w), 7.0, device=_cuda(), dtype=torch.bfloat16)
    del junk
    dx = binding.depthwise_dgrad(torch.zeros_like(dy), wt, (n, c, h, w), st, 1)
    assert torch.count_nonzero(dx).item() == 0


def _module_grads(shape, monkeypatch):
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.conv import Conv2d

    n, h, w, c, st = shape
    x, wt, dy, ref_dx, ref_dw = _case(shape)
    calls = {"dgrad": 0, "wgrad": 0}
    real_d, real_w = binding.depthwise_dgrad, binding.depthwise_wgrad

    def count_d(*a, **k):
        calls["dgrad"] += 1
        return real_d(*a, **k)

    def count_w(*a, **k):
        calls["wgrad"] += 1
        return real_w(*a, **k)

    monkeypatch.setattr(binding, "depthwise_dgrad", count_d)
    monkeypatch.setattr(binding, "depthwise_wgrad", count_w)
    conv = Conv2d(c, c, 3, st, 1, groups=c, bias=False).to(_cuda()).to(torch.bfloat16)
    with torch.no_grad():
        conv.weight.copy_(wt)
    xin = x.detach().clone().requires_grad_()
    y = conv(xin)
    y.backward(dy)
    return calls, xin.grad, conv.weight.grad, ref_dx, ref_dw


@pytest.mark.parametrize("shape", [(3, 20, 20, 96, 1), (2, 15, 15, 24, 2)])
def test_conv2d_depthwise_backward_route(shape, monkeypatch):
    monkeypatch.delenv("DDLW_CONV", raising=False)
    monkeypatch.delenv("DDLW_DISABLE_HIP_OPS", raising=False)
    calls, gx, gw, ref_dx, ref_dw = _module_grads(shape, monkeypatch)
    assert calls == {"dgrad": 1, "wgrad": 1}
    assert gw.dtype == torch.bfloat16 and gx.dtype == torch.bfloat16
    assert _rel(gx, ref_dx) < BOUND
    assert _rel(gw, ref_dw) < BOUND


def test_conv2d_depthwise_backward_honours_needs_input_grad(monkeypatch):
    """A frozen weight asks for no wgrad launch; a leaf input that needs no
    gradient asks for no dgrad launch."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.conv import Conv2d

    monkeypatch.delenv("DDLW_CONV", raising=False)
    monkeypatch.delenv("DDLW_DISABLE_HIP_OPS", raising=False)
    shape = (3, 20, 20, 96, 2)
    n, h, w, c, st = shape
    x, wt, dy, ref_dx, ref_dw = _case(shape)
    calls = []
    real_d, real_w = binding.depthwise_dgrad, binding.depthwise_wgrad
    monkeypatch.setattr(binding, "depthwise_dgrad",
                        lambda *a, **k: (calls.append("d"), real_d(*a, **k))[1])
    monkeypatch.setattr(binding, "depthwise_wgrad",
                        lambda *a, **k: (calls.append("w"), real_w(*a, **k))[1])
    conv = Conv2d(c, c, 3, st, 1, groups=c, bias=False).to(_cuda()).to(torch.bfloat16)
    with torch.no_grad():
        conv.weight.copy_(wt)
    conv(x).backward(dy)                    # input needs no grad
    assert calls == ["w"]
    assert _rel(conv.weight.grad, ref_dw) < BOUND
    calls.clear()
    conv.weight.requires_grad_(False)
    xin = x.detach().clone().requires_grad_()
    conv(xin).backward(dy)                  # weight frozen
    assert calls == ["d"]
    assert _rel(xin.grad, ref_dx) < BOUND


def test_conv2d_depthwise_stock_mode_skips_kernels(monkeypatch):
    monkeypatch.setenv("DDLW_CONV", "stock")
    calls, gx, gw, ref_dx, ref_dw = _module_grads((3, 20, 20, 96, 1), monkeypatch)
    assert calls == {"dgrad": 0, "wgrad": 0}
    assert _rel(gx, ref_dx) < BOUND
    assert _rel(gw, ref_dw) < BOUND
