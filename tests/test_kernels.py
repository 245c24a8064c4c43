"""GPU kernel parity tests: each hand-written HIP op vs a plain PyTorch fp32
reference of the same op. All marked @pytest.mark.gpu.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cuda():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _nhwc_bf16(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn(*shape, generator=g).to(_cuda()).to(torch.bfloat16)
    return _cl(t)


BN_SHAPES = [(4, 64, 56, 56), (2, 256, 28, 28), (3, 2048, 7, 7), (2, 24, 14, 14),
             (2, 2056, 3, 3)]  # vecC = 257: a second, partly idle block column


@pytest.mark.parametrize("shape", BN_SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_bn_act_forward_backward_parity(shape, relu):
    from ddlw_amd.ops.layers import BatchNormAct2d

    n, c, h, w = shape
    torch.manual_seed(0)
    x = _nhwc_bf16(n, c, h, w, seed=1)
    x32 = x.float().detach().requires_grad_(True)
    xb = x.detach().requires_grad_(True)

    layer = BatchNormAct2d(c, relu=relu).to(_cuda())
    layer.train()
    with torch.no_grad():
        layer.weight.uniform_(0.5, 1.5)
        layer.bias.uniform_(-0.5, 0.5)
    ref = torch.nn.BatchNorm2d(c).to(_cuda())
    ref.load_state_dict({k: v for k, v in layer.state_dict().items()}, strict=False)
    ref.train()

    y = layer(xb)
    y_ref = ref(x32)
    if relu:
        y_ref = F.relu(y_ref)
    assert torch.allclose(y.float(), y_ref, atol=5e-2, rtol=5e-2)

    dy = torch.randn_like(y_ref)
    y.backward(dy.to(torch.bfloat16))
    y_ref.backward(dy)
    assert torch.allclose(xb.grad.float(), x32.grad, atol=8e-2, rtol=8e-2)
    assert torch.allclose(layer.weight.grad, ref.weight.grad, atol=2e-1, rtol=2e-2)
    assert torch.allclose(layer.bias.grad, ref.bias.grad, atol=2e-1, rtol=2e-2)
    # running stats updated like the stock op
    assert torch.allclose(layer.running_mean, ref.running_mean, atol=1e-2, rtol=1e-2)
    assert torch.allclose(layer.running_var, ref.running_var, atol=1e-2, rtol=1e-2)


def test_bn_residual_add_relu_parity():
    from ddlw_amd.ops.layers import BatchNormAct2d

    n, c, h, w = 4, 128, 14, 14
    x = _nhwc_bf16(n, c, h, w, seed=2)
    r = _nhwc_bf16(n, c, h, w, seed=3)
    xb = x.detach().requires_grad_(True)
    rb = r.detach().requires_grad_(True)
    x32 = x.float().detach().requires_grad_(True)
    r32 = r.float().detach().requires_grad_(True)

    layer = BatchNormAct2d(c, relu=True).to(_cuda()).train()
    ref = torch.nn.BatchNorm2d(c).to(_cuda()).train()

    y = layer(xb, residual=rb)
    y_ref = F.relu(ref(x32) + r32)
    assert torch.allclose(y.float(), y_ref, atol=5e-2, rtol=5e-2)

    dy = torch.randn_like(y_ref)
    y.backward(dy.to(torch.bfloat16))
    y_ref.backward(dy)
    assert torch.allclose(xb.grad.float(), x32.grad, atol=8e-2, rtol=8e-2)
    assert torch.allclose(rb.grad.float(), r32.grad, atol=5e-2, rtol=5e-2)


def test_bn_eval_mode_parity():
    from ddlw_amd.ops.layers import BatchNormAct2d

    n, c, h, w = 2, 64, 28, 28
    layer = BatchNormAct2d(c, relu=True).to(_cuda())
    with torch.no_grad():
        layer.running_mean.uniform_(-0.3, 0.3)
        layer.running_var.uniform_(0.7, 1.4)
    ref = torch.nn.BatchNorm2d(c).to(_cuda())
    ref.load_state_dict(dict(layer.state_dict()), strict=False)
    layer.eval(), ref.eval()
    x = _nhwc_bf16(n, c, h, w, seed=5)
    xb = x.detach().requires_grad_(True)
    x32 = x.float().detach().requires_grad_(True)
    y = layer(xb)
    y_ref = F.relu(ref(x32))
    assert torch.allclose(y.float(), y_ref, atol=5e-2, rtol=5e-2)
    dy = torch.randn_like(y_ref)
    y.backward(dy.to(torch.bfloat16))
    y_ref.backward(dy)
    assert torch.allclose(xb.grad.float(), x32.grad, atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("shape", [(2, 64, 112, 112), (3, 64, 57, 57)])
def test_maxpool_parity(shape):
    from ddlw_amd.ops.layers import MaxPool3x3s2

    n, c, h, w = shape
    x = _nhwc_bf16(n, c, h, w, seed=7)
    xb = x.detach().requires_grad_(True)
    x32 = x.float().detach().requires_grad_(True)
    y = MaxPool3x3s2()(xb)
    y_ref = F.max_pool2d(x32, 3, stride=2, padding=1)
    assert y.shape == y_ref.shape
    assert torch.allclose(y.float(), y_ref, atol=1e-2, rtol=1e-2)
    dy = torch.randn_like(y_ref)
    y.backward(dy.to(torch.bfloat16))
    y_ref.backward(dy)
    assert torch.allclose(xb.grad.float(), x32.grad, atol=5e-2, rtol=5e-2)


def test_gap_parity():
    from ddlw_amd.ops.layers import GlobalAvgPool2d

    x = _nhwc_bf16(4, 2048, 7, 7, seed=9)
    xb = x.detach().requires_grad_(True)
    x32 = x.float().detach().requires_grad_(True)
    y = GlobalAvgPool2d()(xb)
    y_ref = F.adaptive_avg_pool2d(x32, 1).flatten(1)
    assert torch.allclose(y.float(), y_ref, atol=2e-2, rtol=2e-2)
    dy = torch.randn_like(y_ref)
    y.backward(dy.to(torch.bfloat16))
    y_ref.backward(dy)
    assert torch.allclose(xb.grad.float(), x32.grad, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("C", [5, 33, 1000])
def test_softmax_ce_parity(C):
    """C=5 is the reference's class count; 33 exercises the partial-wave
    column tail; 1000 the bench config."""
    from ddlw_amd.ops.layers import softmax_cross_entropy

    torch.manual_seed(11)
    logits = torch.randn(64, C, device=_cuda()) * 4
    labels = torch.randint(0, C, (64,), device=_cuda())
    l32 = logits.detach().requires_grad_(True)
    lb = logits.detach().requires_grad_(True)
    loss = softmax_cross_entropy(lb, labels)
    loss_ref = F.cross_entropy(l32, labels)
    assert torch.allclose(loss, loss_ref, atol=1e-4, rtol=1e-4)
    loss.backward()
    loss_ref.backward()
    assert torch.allclose(lb.grad, l32.grad, atol=1e-5, rtol=1e-4)


def test_fused_sgd_matches_torch_sgd():
    from ddlw_amd.ops.optim import FusedSGD

    torch.manual_seed(13)
    p1 = [torch.randn(1000, device=_cuda(), requires_grad=True) for _ in range(3)]
    p2 = [p.detach().clone().requires_grad_(True) for p in p1]
    o1 = FusedSGD(p1, lr=0.1, momentum=0.9, weight_decay=1e-4)
    o2 = torch.optim.SGD(p2, lr=0.1, momentum=0.9, weight_decay=1e-4)
    for step in range(3):
        g = [torch.randn(1000, device=_cuda()) for _ in range(3)]
        for a, b, gg in zip(p1, p2, g):
            a.grad = gg.clone()
            b.grad = gg.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)


def test_fused_sgd_bf16_master_mode():
    """bf16 params + bf16 grads: fp32 master semantics must match an fp32
    torch.optim.SGD reference updated with the same (bf16-rounded) grads."""
    from ddlw_amd.ops.optim import FusedSGD

    torch.manual_seed(23)
    base = [torch.randn(512, device=_cuda()) for _ in range(2)]
    p_bf = [b.to(torch.bfloat16).requires_grad_(True) for b in base]
    p_ref = [b.to(torch.bfloat16).float().requires_grad_(True) for b in base]
    o1 = FusedSGD(p_bf, lr=0.05, momentum=0.9, weight_decay=1e-4)
    o2 = torch.optim.SGD(p_ref, lr=0.05, momentum=0.9, weight_decay=1e-4)
    for step in range(4):
        gs = [torch.randn(512, device=_cuda()) for _ in range(2)]
        for a, b, g in zip(p_bf, p_ref, gs):
            a.grad = g.to(torch.bfloat16)
            b.grad = g.to(torch.bfloat16).float()
        o1.step()
        o2.step()
    for a, b, in zip(p_bf, p_ref):
        # bf16 shadow must equal the fp32 reference rounded to bf16
        assert torch.allclose(a.float(), b.to(torch.bfloat16).float(), atol=1e-2, rtol=1e-2)
        master = o1.state[a]["master"]
        assert torch.allclose(master, b, atol=1e-4, rtol=1e-4)


def test_fused_adam_matches_torch_adam():
    from ddlw_amd.ops.optim import FusedAdam

    torch.manual_seed(29)
    p1 = [torch.randn(700, device=_cuda(), requires_grad=True) for _ in range(3)]
    p2 = [p.detach().clone().requires_grad_(True) for p in p1]
    o1 = FusedAdam(p1, lr=1e-3, weight_decay=1e-4)
    o2 = torch.optim.Adam(p2, lr=1e-3, weight_decay=1e-4)
    for step in range(4):
        g = [torch.randn(700, device=_cuda()) for _ in range(3)]
        for a, b, gg in zip(p1, p2, g):
            a.grad = gg.clone()
            b.grad = gg.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)


def test_fused_adam_bf16_master():
    from ddlw_amd.ops.optim import FusedAdam

    torch.manual_seed(31)
    base = torch.randn(512, device=_cuda())
    p_bf = base.to(torch.bfloat16).requires_grad_(True)
    p_ref = base.to(torch.bfloat16).float().requires_grad_(True)
    o1 = FusedAdam([p_bf], lr=1e-2)
    o2 = torch.optim.Adam([p_ref], lr=1e-2)
    for step in range(4):
        g = torch.randn(512, device=_cuda())
        p_bf.grad = g.to(torch.bfloat16)
        p_ref.grad = g.to(torch.bfloat16).float()
        o1.step()
        o2.step()
    assert torch.allclose(o1.state[p_bf]["master"], p_ref, atol=1e-5, rtol=1e-4)
    assert torch.allclose(p_bf.float(), p_ref.to(torch.bfloat16).float(), atol=1e-2, rtol=1e-2)


def test_normalize_u8_parity():
    from ddlw_amd.ops.layers import normalize_u8_bf16

    x = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8).contiguous(
        memory_format=torch.channels_last
    ).to(_cuda())
    y = normalize_u8_bf16(x)
    ref = (x.float() / 127.5) - 1.0
    assert y.dtype == torch.bfloat16
    assert torch.allclose(y.float(), ref, atol=1e-2, rtol=1e-2)


def test_resnet50_hip_step_runs_and_matches_loss_scale():
    """End-to-end: one fwd+bwd+opt step of ResNet-50 with every HIP op active;
    loss must be finite and near ln(1000) at random init."""
    import math

    from ddlw_amd.models import build_resnet50
    from ddlw_amd.ops import FusedSGD, softmax_cross_entropy

    torch.manual_seed(17)
    model = build_resnet50(num_classes=1000).to(_cuda()).to(memory_format=torch.channels_last)
    for m in model.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            m.to(torch.bfloat16)
    opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9)
    x = _nhwc_bf16(8, 3, 224, 224, seed=19)
    ylab = torch.randint(0, 1000, (8,), device=_cuda())
    model.train()
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        logits = model(x)
        loss = softmax_cross_entropy(logits, ylab)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(math.isfinite(l) for l in losses)
    assert abs(losses[0] - math.log(1000)) < 1.0
    assert losses[-1] < losses[0] + 0.5  # training on a fixed batch shouldn't blow up


def test_native_lib_is_loaded():
    """The round-end check looks for the in-tree .so in loaded maps — assert
    the HIP library really is what runs (no silent eager fallback)."""
    from ddlw_amd.ops import require_lib
    from ddlw_amd.ops.runtime import LIB_DIR, LIB_NAME

    require_lib()
    maps = open("/proc/self/maps").read()
    assert str(LIB_DIR / LIB_NAME) in maps


def test_training_equivalence_hip_vs_stock():
    """8 training steps of ResNet-50 on a fixed batch: the full ddlw path
    (bf16 weights, every HIP kernel + FusedSGD) must track the stock fp32
    path's loss trajectory — an end-to-end numerics gate beyond per-kernel
    parity."""
    import os

    from ddlw_amd.models import build_resnet50
    from ddlw_amd.ops import FusedSGD, softmax_cross_entropy

    torch.manual_seed(99)
    x32 = torch.randn(16, 3, 64, 64, device=_cuda())
    y = torch.randint(0, 10, (16,), device=_cuda())

    def run(hip: bool):
        os.environ["DDLW_DISABLE_HIP_OPS"] = "0" if hip else "1"
        os.environ["DDLW_CONV"] = "hip" if hip else "stock"
        try:
            torch.manual_seed(7)
            m = build_resnet50(num_classes=10).to(_cuda())
            losses = []
            if hip:
                m = m.to(memory_format=torch.channels_last)
                for mod in m.modules():
                    if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
                        mod.to(torch.bfloat16)
                opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9)
                xb = x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                for _ in range(8):
                    opt.zero_grad(set_to_none=True)
                    loss = softmax_cross_entropy(m(xb), y)
                    loss.backward()
                    opt.step()
                    losses.append(float(loss.detach()))
            else:
                opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
                for _ in range(8):
                    opt.zero_grad(set_to_none=True)
                    loss = torch.nn.functional.cross_entropy(m(x32), y)
                    loss.backward()
                    opt.step()
                    losses.append(float(loss))
            return losses
        finally:
            os.environ.pop("DDLW_DISABLE_HIP_OPS", None)
            os.environ.pop("DDLW_CONV", None)

    ref = run(False)
    hip = run(True)
    # same init/seed/batch: trajectories must track (bf16 vs fp32 tolerance)
    assert abs(hip[0] - ref[0]) / max(ref[0], 1e-6) < 0.05, (hip[0], ref[0])
    # loss must be decreasing on the fixed batch in both paths
    assert hip[-1] < hip[0] and ref[-1] < ref[0], (hip, ref)
    for a, b in zip(hip, ref):
        assert abs(a - b) / max(abs(b), 0.3) < 0.35, (hip, ref)



def test_dropout_kernel_stats_and_determinism():
    """K7: keep-rate ~ (1-p), kept values scaled 1/(1-p), deterministic per
    seed, and backward zeroes exactly the dropped positions."""
    from ddlw_amd.ops import binding

    torch.manual_seed(11)
    x = torch.randn(64, 1280, device="cuda").to(torch.bfloat16).abs() + 0.5
    p = 0.37
    y1, m1 = binding.dropout_fwd(x, p, seed=1234)
    y2, m2 = binding.dropout_fwd(x, p, seed=1234)
    assert torch.equal(y1, y2) and torch.equal(m1, m2)  # deterministic
    y3, _ = binding.dropout_fwd(x, p, seed=99)
    assert not torch.equal(y1, y3)  # seed-dependent
    kept = (y1 != 0)
    rate = kept.float().mean().item()
    assert abs(rate - (1 - p)) < 0.02, rate
    scale = (y1.float()[kept] / x.float()[kept])
    assert ((scale - 1 / (1 - p)).abs() < 0.02).all()
    dy = torch.ones_like(x)
    dx = binding.dropout_bwd(dy, m1, p)
    assert torch.equal((dx != 0), kept)  # same mask both ways


def test_dropout_module_autograd():
    from ddlw_amd.ops.layers import Dropout

    torch.manual_seed(3)
    d = Dropout(0.5).train()
    x = torch.randn(8, 1280, device="cuda").to(torch.bfloat16).requires_grad_(True)
    y = d(x)
    y.float().sum().backward()
    # grad nonzero exactly where output nonzero
    assert torch.equal((x.grad != 0), (y != 0))
    d.eval()
    assert torch.equal(d(x), x)  # identity in eval


def test_argmax_and_accuracy_kernels():
    """K11/K12 vs torch (incl. first-max tie-break)."""
    from ddlw_amd.ops import binding

    torch.manual_seed(5)
    for C in (5, 33, 1000):
        logits = torch.randn(257, C, device="cuda")
        logits[0, :] = 1.0  # all-ties row: torch picks index 0
        idx = binding.argmax_rows(logits)
        assert torch.equal(idx, logits.argmax(-1))
        labels = torch.randint(0, C, (257,), device="cuda")
        acc = binding.accuracy(logits, labels)
        ref = (logits.argmax(-1) == labels).float().mean()
        assert torch.allclose(acc, ref), (C, acc, ref)
