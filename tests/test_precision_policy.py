"""``train.Model(precision="bf16")`` on the GPU: the facade computes what the
hand recipe computes, bit for bit, and reaches the hand-written kernels."""
import copy

import pytest
import torch

from ddlw_amd.models import build_model, build_resnet50

ENV_SWITCHES = ("DDLW_DISABLE_HIP_OPS", "DDLW_EVAL_FOLD", "DDLW_CONV",
                "DDLW_STEM_U8", "DDLW_PW_TRAIN")


def _dev():
    return torch.device("cuda:0")


def _clear_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _u8(n, size=32, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g)


def _randomize_bn(model, seed):
    """Frozen BN with running stats of a trained net, not the (0, 1) init."""
    from ddlw_amd.ops.layers import BatchNormAct2d

    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, BatchNormAct2d):
                for t, lo, hi in ((mod.running_mean, -0.3, 0.3), (mod.running_var, 0.5, 1.5),
                                  (mod.weight, 0.5, 1.5), (mod.bias, -0.2, 0.2)):
                    t.copy_(torch.empty_like(t, device="cpu").uniform_(lo, hi, generator=g))


def _count_calls(monkeypatch, names):
    from ddlw_amd.ops import binding

    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(binding, n)

        def counted(*a, _real=real, _n=n, **k):
            calls[_n] += 1
            return _real(*a, **k)

        monkeypatch.setattr(binding, n, counted)
    return calls


def _model(seed=31, **kw):
    torch.manual_seed(seed)
    m = build_model(32, 32, 3, 5, dropout=0.0, **kw)
    _randomize_bn(m, seed=9)
    return m


@pytest.mark.gpu
def test_facade_predict_equals_hand_recipe(monkeypatch):
    from ddlw_amd.ops import apply_bf16_policy
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    m = _model()
    m2 = copy.deepcopy(m)
    u8 = _u8(4)

    model = Model(m, _dev(), precision="bf16")
    assert model.precision == "bf16"
    assert m.classifier.weight.dtype == torch.bfloat16 and m.classifier.weight.is_cuda
    out = model.predict(u8)
    assert out.dtype == torch.float32 and out.device.type == "cpu"
    assert out.shape == (4, 5) and torch.isfinite(out).all()
    out.numpy()  # fp32 logits: numpy takes them

    hand = apply_bf16_policy(m2.to(_dev())).eval()
    with torch.no_grad():
        ref = hand(u8.to(_dev()).permute(0, 3, 1, 2)).float().cpu()
    assert torch.equal(out, ref)
    # the same batch as the N x C x H x W channels_last view, host or device
    assert torch.equal(model.predict(u8.permute(0, 3, 1, 2)), ref)
    assert torch.equal(model.predict(u8.to(_dev()).permute(0, 3, 1, 2)), ref)


@pytest.mark.gpu
def test_facade_train_step_equals_hand_loop(monkeypatch):
    """Batch 2: the loss kernel sums rows with atomics, and a sum of two is
    the one size whose result cannot depend on their order."""
    from ddlw_amd.ops import FusedAdam, apply_bf16_policy, softmax_cross_entropy
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    m = _model(seed=33)
    m2 = copy.deepcopy(m)
    u8 = _u8(2, seed=7)
    labels = torch.tensor([1, 3])

    model = Model(m, _dev(), precision="bf16").compile("Adam")
    assert isinstance(model.optimizer, FusedAdam)
    w_start = m.classifier.weight.detach().clone()
    logs = model.train_step(u8, labels)

    hand = apply_bf16_policy(m2.to(_dev())).train()
    opt = FusedAdam([p for p in hand.parameters() if p.requires_grad], lr=1e-3)
    opt.zero_grad(set_to_none=True)
    loss = softmax_cross_entropy(hand(u8.to(_dev()).permute(0, 3, 1, 2)), labels.to(_dev()))
    loss.backward()
    opt.step()
    assert logs["loss"] == float(loss.detach())
    assert m.classifier.weight.dtype == torch.bfloat16
    assert torch.equal(m.classifier.weight, hand.classifier.weight)
    assert not torch.equal(opt.state[hand.classifier.weight]["master"], w_start.float())
    assert torch.equal(model.optimizer.state[m.classifier.weight]["master"],
                       opt.state[hand.classifier.weight]["master"])


@pytest.mark.gpu
def test_facade_route_reaches_the_kernels(monkeypatch):
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    names = ("stem3_u8_fwd_ep", "pw_conv_fwd", "normalize_u8")
    m = _model()
    m32 = copy.deepcopy(m).to(_dev())
    u8 = _u8(4)

    model = Model(m, _dev(), precision="bf16")
    calls = _count_calls(monkeypatch, names)
    model.predict(u8)
    assert calls["stem3_u8_fwd_ep"] >= 1 and calls["pw_conv_fwd"] >= 1, calls
    assert calls["normalize_u8"] == 0, calls

    model32 = Model(m32, _dev(), precision="fp32")
    for k in calls:
        calls[k] = 0
    out = model32.predict(u8.permute(0, 3, 1, 2))
    assert out.dtype == torch.float32
    assert calls == {n: 0 for n in names}, calls
    assert m32.classifier.weight.dtype == torch.float32


@pytest.mark.gpu
def test_facade_finetune_step_and_optimizer_names(monkeypatch):
    from ddlw_amd.ops import FusedAdadelta, FusedAdam, FusedSGD
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    m = _model(fine_tune_at=17)
    grad_before = {k: p.requires_grad for k, p in m.named_parameters()}
    model = Model(m, _dev(), precision="bf16")
    assert {k: p.requires_grad for k, p in m.named_parameters()} == grad_before

    with pytest.raises(ValueError, match="Adadelta"):
        model.compile("AdamW")
    assert isinstance(model.compile("SGD").optimizer, FusedSGD)
    assert isinstance(model.compile("Adam").optimizer, FusedAdam)
    model.compile("Adadelta", learning_rate=1.0)
    assert isinstance(model.optimizer, FusedAdadelta)
    n_trainable = sum(1 for v in grad_before.values() if v)
    assert len(model.optimizer.param_groups[0]["params"]) == n_trainable

    calls = _count_calls(monkeypatch, ("pw_conv_fwd_stats", "depthwise_dgrad",
                                       "fused_adadelta", "stem3_u8_fwd_ep"))
    w0 = m.classifier.weight.detach().clone()
    logs = model.train_step(_u8(4), torch.tensor([0, 1, 2, 3]))
    assert calls["pw_conv_fwd_stats"] >= 1 and calls["depthwise_dgrad"] >= 1, calls
    assert calls["fused_adadelta"] == 1 and calls["stem3_u8_fwd_ep"] == 1, calls
    assert logs["loss"] == logs["loss"] and abs(logs["loss"]) < float("inf"), logs
    assert 0.0 <= logs["accuracy"] <= 1.0
    # every trainable parameter got an fp32 state and bf16 ones a master
    for p in model.optimizer.param_groups[0]["params"]:
        st = model.optimizer.state[p]
        assert st["square_avg"].dtype == torch.float32
        assert ("master" in st) == (p.dtype == torch.bfloat16)
    assert not torch.equal(model.optimizer.state[m.classifier.weight]["master"], w0.float())
    ev = model.eval_step(_u8(4), torch.tensor([0, 1, 2, 3]))
    assert abs(ev["loss"]) < float("inf")


@pytest.mark.gpu
def test_facade_float_batch_close_to_fp32(monkeypatch):
    """bf16 against fp32 with the bounds of tests/test_kernels.py (5e-2)."""
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    m = _model()
    m32 = copy.deepcopy(m).to(_dev())
    x = _u8(4).permute(0, 3, 1, 2).float() / 127.5 - 1.0  # fp32 NCHW
    ref = Model(m32, _dev(), precision="fp32").predict(x)
    out = Model(m, _dev(), precision="bf16").predict(x)
    err = (out - ref).abs().max().item()
    print(f"bf16 vs fp32 logits: max abs {err:.4e}, ref max {ref.abs().max().item():.4e}")
    assert out.dtype == torch.float32
    assert torch.allclose(out, ref, atol=5e-2, rtol=5e-2), err


@pytest.mark.gpu
def test_facade_module_without_accepts_uint8(monkeypatch):
    from ddlw_amd.ops import apply_bf16_policy, normalize_u8_bf16
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    torch.manual_seed(35)
    r = build_resnet50(num_classes=5)
    assert not getattr(r, "accepts_uint8", False)
    r2 = copy.deepcopy(r)
    u8 = _u8(2)
    calls = _count_calls(monkeypatch, ("normalize_u8",))
    out = Model(r, _dev(), precision="bf16").predict(u8)
    assert calls["normalize_u8"] == 1, calls
    hand = apply_bf16_policy(r2.to(_dev())).eval()
    with torch.no_grad():
        ref = hand(normalize_u8_bf16(u8.to(_dev()).permute(0, 3, 1, 2))).float().cpu()
    assert out.dtype == torch.float32 and torch.equal(out, ref)


@pytest.mark.gpu
def test_auto_resolves_to_bf16_on_gpu(monkeypatch):
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    m = _model()
    model = Model(m, _dev(), precision="auto")
    assert model.precision == "bf16"
    assert m.classifier.weight.dtype == torch.bfloat16
