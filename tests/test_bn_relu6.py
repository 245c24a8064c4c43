"""Fused BN + ReLU6 (BatchNormAct2d(act="relu6")): CPU fallback semantics and
GPU kernel parity against F.relu6(nn.BatchNorm2d) in fp32."""
import pytest
import torch
import torch.nn.functional as F


def _pair(c, **kw):
    from ddlw_amd.ops.layers import BatchNormAct2d

    a, b = BatchNormAct2d(c, **kw), BatchNormAct2d(c)
    with torch.no_grad():
        a.weight.uniform_(2.0, 4.0)
        a.bias.uniform_(2.0, 4.0)
        a.running_mean.uniform_(-0.5, 0.5)
        a.running_var.uniform_(0.5, 1.5)
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("train", [True, False])
def test_relu6_cpu_matches_bn_then_relu6(train):
    torch.manual_seed(0)
    a, b = _pair(16, act="relu6")
    a.train(train), b.train(train)
    x = torch.randn(4, 16, 9, 9)
    ya, yb = a(x), F.relu6(b(x))
    assert torch.equal(ya, yb)
    assert ya.max().item() == 6.0 and ya.min().item() == 0.0
    assert torch.equal(a.running_mean, b.running_mean)
    assert torch.equal(a.running_var, b.running_var)


@pytest.mark.parametrize("train", [True, False])
def test_relu_bool_unchanged_cpu(train):
    from ddlw_amd.ops.layers import BatchNormAct2d

    torch.manual_seed(1)
    a, b = _pair(16, relu=True)
    a.train(train), b.train(train)
    x = torch.randn(4, 16, 9, 9)
    assert a.relu is True and a.act == "relu"
    assert b.relu is False and b.act == "none"
    assert torch.equal(a(x), F.relu(b(x)))
    assert torch.equal(BatchNormAct2d(16, act="relu").eval()(x),
                       BatchNormAct2d(16, relu=True).eval()(x))
    r6 = BatchNormAct2d(16, act="relu6")
    assert r6.relu is False  # `relu` keeps meaning "a plain ReLU is fused"
    assert list(r6.state_dict()) == list(b.state_dict())


def test_unknown_act_rejected():
    from ddlw_amd.ops.layers import BatchNormAct2d

    with pytest.raises(ValueError):
        BatchNormAct2d(8, act="gelu")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 24, 14, 14), (4, 64, 28, 28)])
def test_bn_relu6_forward_backward_parity(shape):
    """Tolerances are those of test_bn_act_forward_backward_parity. gamma and
    beta ~3 put the pre-activation at ~N(3, 3^2): ~16% below 0, ~68% inside
    (0, 6), ~16% above 6."""
    from ddlw_amd.ops.layers import BatchNormAct2d

    dev = torch.device("cuda:0")
    n, c, h, w = shape
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(n, c, h, w, generator=g).to(dev).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    x32 = x.float().detach().requires_grad_(True)
    xb = x.detach().requires_grad_(True)

    layer = BatchNormAct2d(c, act="relu6").to(dev).train()
    torch.manual_seed(0)
    with torch.no_grad():
        layer.weight.uniform_(2.8, 3.2)
        layer.bias.uniform_(2.8, 3.2)
    ref = torch.nn.BatchNorm2d(c).to(dev)
    ref.load_state_dict(dict(layer.state_dict()), strict=False)
    ref.train()

    pre = ref(x32)
    y_ref = F.relu6(pre)
    numel = pre.numel()
    for name, cnt in (("<0", (pre < 0).sum()), ("(0,6)", ((pre > 0) & (pre < 6)).sum()),
                      (">6", (pre > 6).sum())):
        share = cnt.item() / numel
        print(f"{shape} region {name}: {share:.3f}")
        assert share >= 0.05, (name, share)

    y = layer(xb)
    assert torch.allclose(y.float(), y_ref, atol=5e-2, rtol=5e-2)
    assert y.max().item() == 6.0 and y.min().item() == 0.0

    dy = torch.randn(y_ref.shape, generator=g).to(dev)
    y.backward(dy.to(torch.bfloat16))
    y_ref.backward(dy)
    # a bf16-rounded input can land on the other side of a kink than the fp32
    # reference only when the reference sits within 1e-2 of that kink
    near = ((pre.detach().abs() < 1e-2) | ((pre.detach() - 6).abs() < 1e-2))
    # dx of one element depends on every element of its channel through the
    # batch statistics, but only the element's own mask bit can flip its
    # leading term; exclude exactly those
    excluded = near.float().mean().item()
    print(f"{shape} excluded share {excluded:.4f}")
    assert excluded <= 0.01
    keep = ~near
    assert torch.allclose(xb.grad.float()[keep], x32.grad[keep], atol=8e-2, rtol=8e-2)
    assert torch.allclose(layer.weight.grad, ref.weight.grad, atol=2e-1, rtol=2e-2)
    assert torch.allclose(layer.bias.grad, ref.bias.grad, atol=2e-1, rtol=2e-2)
    assert torch.allclose(layer.running_mean, ref.running_mean, atol=1e-2, rtol=1e-2)
    assert torch.allclose(layer.running_var, ref.running_var, atol=1e-2, rtol=1e-2)


@pytest.mark.gpu
def test_bn_relu6_mask_matches_hardtanh_rule():
    """Mask bit set iff 0 < f < 6 on the fp32 value: elements clamped at 0 or
    6 get exactly zero gradient (eval mode, so dx = gamma*rstd*dy*mask)."""
    from ddlw_amd.ops.layers import BatchNormAct2d

    dev = torch.device("cuda:0")
    layer = BatchNormAct2d(8, act="relu6").to(dev).eval()
    vals = torch.tensor([-3.0, -0.5, 0.0, 0.5, 3.0, 5.5, 6.0, 9.0], device=dev)
    x = vals.view(1, 1, 8, 1).expand(1, 8, 8, 1).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    layer.eps = 0.0  # running stats (0, 1) -> y = relu6(x) exactly
    y = layer(x)
    assert torch.equal(y.float(), F.relu6(x.detach().float()))
    y.backward(torch.ones_like(y))
    expect = ((vals > 0) & (vals < 6)).float().view(1, 1, 8, 1).expand(1, 8, 8, 1)
    assert torch.equal(x.grad.float(), expect)
