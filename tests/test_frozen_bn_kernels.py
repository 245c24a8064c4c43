"""The gated backward kernels of a conv + frozen-BN stage
(``hip/pointwise_frozen.hip``, ``k_depthwise_bwd_gated``) against fp64, and a
block on them against the module path.

Reference: fp64 sums over the same bf16 operands, with ``g16 = gate(out) ?
bf16(fp32(dout) * scale) : 0`` built in torch as the kernels define it. bf16
products are exact in fp32, so only the fp32 accumulation (depth D: D * 2^-23
of the sum of magnitudes) and the one rounding to bf16 (2^-8 relative; none
for the fp32 depthwise dW) contribute.
"""
import copy

import pytest
import torch

R, E = 2.0 ** -8, 2.0 ** -23


def _within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    print(f"{what}: max err / bound = {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), what


def _stage(shape, K, act, seed, lone=False):
    """dout, out, scale and g16 of a stage output of ``shape`` (channels K on
    dim 1 or last). ``out`` holds exact 0.0 and 6.0 (both gate edges, closed);
    ``lone``: dout is zero but for one element, on the 0.0."""
    g = torch.Generator().manual_seed(seed)
    numel = torch.Size(shape).numel()
    dout = torch.randn(shape, generator=g) / (numel // K)
    out = (3 * torch.randn(shape, generator=g) + 3).to(torch.bfloat16)
    out.view(-1)[0], out.view(-1)[-1] = 0.0, 6.0
    if lone:
        dout.zero_().view(-1)[0] = 1.0
    dout = dout.to(torch.bfloat16)
    scale = (0.5 + torch.rand(K, generator=g)) * torch.where(torch.rand(K, generator=g) < 0.3, -1.0, 1.0)
    sc = scale.view(1, K, 1, 1) if len(shape) == 4 else scale
    g16 = (dout.float() * sc).to(torch.bfloat16)
    if act == 2:
        g16 = torch.where((out > 0) & (out < 6), g16, torch.zeros_like(g16))
    return dout, out, scale, g16.double()


PW_SHAPES = [(1, 8, 8), (37, 24, 40), (130, 40, 8), (98, 160, 960)]


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("M, C, K", PW_SHAPES + [(3 * 64 + 5, 24, 40)])  # + wgrad: 3 slices and a tail
def test_pointwise_against_fp64(M, C, K, with_acc, act):
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import query

    dev = torch.device("cuda:0")
    dout, out, scale, g16 = _stage((M, K), K, act, M * 131 + C * 7 + K)
    g = torch.Generator().manual_seed(M + C + K)
    x = torch.randn(M, C, generator=g).to(torch.bfloat16)
    w = (0.1 * torch.randn(K, C, 1, 1, generator=g)).to(torch.bfloat16)
    acc = torch.randn(M, C, generator=g).to(torch.bfloat16) / M if with_acc else None
    wd, xd = w.view(K, C).double(), x.double()
    what = f"M{M} C{C} K{K} act{act}"
    to = lambda t: None if t is None else t.to(dev)

    args = (to(dout), to(out), to(w), to(scale), act, (M, C), to(acc))
    dx = binding.pw_dgrad_gated(*args)
    ref, mag = g16 @ wd, g16.abs() @ wd.abs()
    if with_acc:
        ref, mag = ref + acc.double(), mag + acc.double().abs()
    _within(dx, ref, R * ref.abs() + K * E * mag, what + " dx")
    assert torch.equal(dx, binding.pw_dgrad_gated(*args))

    if M == 3 * 64 + 5:
        assert query("pw_wgrad_gated_nparts", M, C, K, None) == 4
    args = (to(dout), to(out), to(x), to(scale), act, (K, C, 1, 1))
    dw = binding.pw_wgrad_gated(*args)
    ref = g16.t() @ xd
    _within(dw.view(K, C), ref, R * ref.abs() + M * E * (g16.abs().t() @ xd.abs()), what + " dW")
    assert dw.dtype == torch.bfloat16 and torch.equal(dw, binding.pw_wgrad_gated(*args))


DW_SHAPES = [(1, 1, 1, 8, 1), (2, 9, 7, 24, 1), (1, 17, 9, 8, 1), (1, 7, 9, 8, 2),
             (1, 10, 10, 40, 2)]


def _dw_ref(x, w, g16, stride):
    """(dx, dW) in fp64 of sum(conv(x, w) * g16)."""
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = torch.nn.functional.conv2d(x, w, stride=stride, padding=1, groups=w.shape[0])
    (y * g16).sum().backward()
    return x.grad, w.grad


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("N, H, W, C, stride", DW_SHAPES)
def test_depthwise_against_fp64(N, H, W, C, stride, need_dx, act):
    from ddlw_amd.ops import binding

    dev = torch.device("cuda:0")
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dout, out, scale, g16 = _stage((N, C, ho, wo), C, act, H * 131 + W * 7 + C + stride)
    g = torch.Generator().manual_seed(H + W + C)
    x = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16)
    w = (0.3 * torch.randn(C, 1, 3, 3, generator=g)).to(torch.bfloat16)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    args = (cl(dout), cl(out), cl(x), w.to(dev), scale.to(dev), act, stride, need_dx)
    dx, dw = binding.depthwise_bwd_gated(*args)
    again = binding.depthwise_bwd_gated(*args)
    rx, rw = _dw_ref(x.double(), w.double(), g16, stride)
    mx, mw = _dw_ref(x.double().abs(), w.double().abs(), g16.abs(), stride)
    what = f"N{N} {H}x{W} C{C} s{stride} act{act}"
    _within(dw, rw, N * ho * wo * E * mw, what + " dW")
    assert dw.dtype == torch.float32 and torch.equal(dw, again[1])
    assert (dx is None) == (not need_dx)
    if need_dx:
        _within(dx, rx, R * rx.abs() + 9 * E * mx, what + " dx")
        assert torch.equal(dx, again[0])


@pytest.mark.gpu
def test_a_closed_gate_passes_nothing():
    """One nonzero dout element, on an ``out`` of exactly 0.0: every gradient
    is exactly zero."""
    from ddlw_amd.ops import binding

    dev = torch.device("cuda:0")
    dout, out, scale, _ = _stage((37, 40), 40, 2, 1, lone=True)
    x = torch.randn(37, 24).to(torch.bfloat16).to(dev)
    w = torch.randn(40, 24, 1, 1).to(torch.bfloat16).to(dev)
    dout, out, scale = dout.to(dev), out.to(dev), scale.to(dev)
    assert not binding.pw_dgrad_gated(dout, out, w, scale, 2, (37, 24)).any()
    assert not binding.pw_wgrad_gated(dout, out, x, scale, 2, (40, 24, 1, 1)).any()
    assert binding.pw_dgrad_gated(dout, out, w, scale, 0, (37, 24)).any()
    for stride in (1, 2):
        dout, out, scale, _ = _stage((1, 8, 5, 5), 8, 2, 2, lone=True)
        cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
        x = cl(torch.randn(1, 8, 5 * stride, 5 * stride).to(torch.bfloat16))
        w = torch.randn(8, 1, 3, 3).to(torch.bfloat16).to(dev)
        dx, dw = binding.depthwise_bwd_gated(cl(dout), cl(out), x, w, scale.to(dev), 2, stride, True)
        assert not dx.any() and not dw.any()


def _grads(block, x, dout):
    x = x.clone().requires_grad_()
    (block(x) * dout).sum().backward()
    return [x.grad] + [m.weight.grad for m in block.conv if hasattr(m, "kernel_size")]


@pytest.mark.gpu
@pytest.mark.parametrize("cin, cout, stride", [(16, 16, 1), (16, 24, 2)])
def test_block_against_the_module_path(monkeypatch, cin, cout, stride):
    """Gradients (input, three conv weights) of a frozen-BN block under
    ``DDLW_FROZEN_BN=1`` and ``=0``, each against an fp64 copy by relative L2
    error. The two bf16 paths round at different points and neither
    dominates, so no margin can be derived: the fused path's error may be at
    most twice the module path's."""
    from ddlw_amd.models.mobilenet_v2 import InvertedResidual
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.layers import BatchNormAct2d

    torch.manual_seed(cin + cout)
    ref = InvertedResidual(cin, cout, stride, 6).double().eval()
    for m in ref.modules():
        if isinstance(m, BatchNormAct2d):
            m.running_mean.normal_(0, 0.5), m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5), m.bias.data.normal_(0, 0.5)
            m.weight.requires_grad = m.bias.requires_grad = False
        elif hasattr(m, "kernel_size"):
            m.weight.data = m.weight.data.bfloat16().double()
    blk = copy.deepcopy(ref).float().to("cuda:0").to(memory_format=torch.channels_last)
    for m in blk.modules():
        if hasattr(m, "kernel_size"):
            m.to(torch.bfloat16)
    x = torch.randn(2, cin, 9, 9).bfloat16()
    ho = (9 - 1) // stride + 1
    dout = torch.randn(2, cout, ho, ho).bfloat16()
    want = _grads(ref, x.double(), dout.double())
    xg = x.to("cuda:0").contiguous(memory_format=torch.channels_last)
    dg = dout.to("cuda:0").contiguous(memory_format=torch.channels_last)

    calls = []
    for name in ("pw_dgrad_gated", "pw_wgrad_gated", "depthwise_bwd_gated"):
        real = getattr(binding, name)
        monkeypatch.setattr(binding, name,
                            lambda *a, _r=real, _n=name: (calls.append(_n), _r(*a))[1])
    err = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DDLW_FROZEN_BN", mode)
        del calls[:]
        got = _grads(copy.deepcopy(blk), xg, dg)
        assert set(calls) == ({"pw_dgrad_gated", "pw_wgrad_gated", "depthwise_bwd_gated"}
                              if mode == "1" else set())
        err[mode] = [((g.double().cpu() - r).norm() / r.norm()).item() for g, r in zip(got, want)]
    for what, e1, e0 in zip(("dx", "dW expand", "dW depthwise", "dW project"), err["1"], err["0"]):
        print(f"s{stride} {what}: fused {e1:.3e}, module {e0:.3e}, ratio {e1 / e0:.2f}")
        assert e1 <= 2 * e0, what
