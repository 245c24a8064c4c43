"""``fine_tune_at``: the frozen/trainable split of the MobileNetV2 transfer
model, and on the GPU the gradients of the trainable suffix through the
hand-written depthwise backward and fused BN+ReLU6 kernels."""
import copy

import pytest
import torch

from ddlw_amd.core import tracking
from ddlw_amd.core.model_io import load_model, log_model
from ddlw_amd.models import build_model

HEAD = 1280 * 5 + 5
N_KEYS = 314  # state_dict entries of the transfer model before fine_tune_at existed


def _trainable(m):
    return sum(p.numel() for p in m.parameters() if p.requires_grad)


def _flags(m):
    return [(n, p.requires_grad) for n, p in m.named_parameters()]


def _feats(m):
    return m.base.base.features


def test_default_none_and_23_are_the_frozen_model():
    models = [build_model(num_classes=5), build_model(num_classes=5, fine_tune_at=None),
              build_model(num_classes=5, fine_tune_at=23)]
    keys = [list(m.state_dict()) for m in models]
    assert keys[0] == keys[1] == keys[2]
    assert len(keys[0]) == N_KEYS
    for k in ("base.base.features.0.weight", "base.base.features.21.running_mean",
              "base.base.features.1.num_batches_tracked",
              "base.base.features.3.conv.0.weight",
              "base.base.features.4.conv.4.running_var",
              "base.base.features.19.conv.7.bias", "classifier.weight", "classifier.bias"):
        assert k in keys[0], k
    assert len(_feats(models[0])) == 23
    for m in models:
        assert _trainable(m) == HEAD
        m.train()
        assert all(not mod.training for mod in m.base.base.modules())
        x = torch.randn(2, 3, 64, 64)
        y = m(x)
        assert y.shape == (2, 5)
        y.sum().backward()
        assert all(p.grad is None for p in m.base.parameters())
        assert m.classifier.weight.grad is not None


def test_fine_tune_at_20_split():
    m = build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=20)
    assert _trainable(m) == HEAD + 320 * 1280 + 2 * 1280
    m.train()
    feats = _feats(m)
    for i, child in enumerate(feats):
        for mod in child.modules():
            assert mod.training == (i >= 20), i
    rm_frozen = feats[1].running_mean.clone()
    rm_live = feats[21].running_mean.clone()
    m(torch.randn(4, 3, 64, 64)).sum().backward()
    assert feats[20].weight.grad is not None
    assert feats[21].weight.grad is not None
    assert all(p.grad is None for p in feats[19].parameters())
    assert all(p.grad is None for p in feats[0].parameters())
    # frozen BN keeps its moving statistics, trainable BN uses the batch
    assert torch.equal(feats[1].running_mean, rm_frozen)
    assert not torch.equal(feats[21].running_mean, rm_live)
    m.eval()
    assert all(not mod.training for mod in m.modules())


@pytest.mark.parametrize("bad", [24, -1, 2.0, True])
def test_fine_tune_at_out_of_range(bad):
    with pytest.raises(ValueError):
        build_model(num_classes=5, fine_tune_at=bad)
    m = build_model(num_classes=5)
    with pytest.raises(ValueError):
        m.set_fine_tune_at(bad)


def test_set_fine_tune_at_equals_building_with_it():
    built = build_model(num_classes=5, fine_tune_at=16)
    later = build_model(num_classes=5)
    later.train()
    later.set_fine_tune_at(16)
    assert _flags(later) == _flags(built)
    built.train()
    assert [m.training for m in later.modules()] == [m.training for m in built.modules()]
    later.set_fine_tune_at(None)
    assert _trainable(later) == HEAD
    assert all(not mod.training for mod in later.base.base.modules())
    later.set_fine_tune_at(0)
    assert all(p.requires_grad for p in later.parameters())


def test_fine_tune_at_save_load_roundtrip(ddlw_home):
    tracking.set_experiment("finetune")
    m = build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=16)
    with tracking.start_run():
        uri = log_model(m, "model")
    m2 = load_model(uri)
    assert m2.base.fine_tune_at == 16
    assert _flags(m2) == _flags(m)
    x = torch.randn(2, 3, 64, 64)
    m.eval(), m2.eval()
    assert torch.allclose(m(x), m2(x), atol=1e-6)
    # a split switched on after building is saved too
    m3 = build_model(64, 64, 3, 5, dropout=0.0)
    m3.set_fine_tune_at(20)
    with tracking.start_run():
        uri3 = log_model(m3, "model")
    assert _flags(load_model(uri3)) == _flags(m3)


# --------------------------------------------------------------------------- #
# GPU: gradients of the trainable suffix
# --------------------------------------------------------------------------- #


def _grads(model, x, labels, monkeypatch, env, bf16):
    from ddlw_amd.ops.layers import softmax_cross_entropy

    for k in ("DDLW_CONV", "DDLW_DISABLE_HIP_OPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = copy.deepcopy(model).to(memory_format=torch.channels_last)
    if bf16:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
    m.train()
    loss = softmax_cross_entropy(m(x.contiguous(memory_format=torch.channels_last)), labels)
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().float() for n, p in m.named_parameters() if p.requires_grad}


@pytest.mark.gpu
def test_finetune_gradients_vs_library_pipeline(monkeypatch):
    """One forward+backward of build_model(64,64,3,5,fine_tune_at=13), batch
    8: depthwise C=384/576/960 at 4x4 and 2x2, one of them stride 2.

    Three gradient sets from identical weights and input: G32 (fp32, stock
    ops), Glib (bf16, DDLW_CONV=stock) and Ghip (bf16, default route). Per
    trainable tensor the relative L2 error to G32 must satisfy
    err(Ghip) <= 2*err(Glib) + 1e-3: the library pipeline is the yardstick,
    and 2x covers two bf16 pipelines that round in different orders.
    """
    from ddlw_amd.ops import binding

    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=13).to(dev)
    x = torch.randn(8, 3, 64, 64, device=dev)
    labels = torch.randint(0, 5, (8,), device=dev)

    g32 = _grads(model, x, labels, monkeypatch, {"DDLW_DISABLE_HIP_OPS": "1"}, bf16=False)
    glib = _grads(model, x, labels, monkeypatch, {"DDLW_CONV": "stock"}, bf16=True)

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
    ghip = _grads(model, x, labels, monkeypatch, {}, bf16=True)
    assert calls["dgrad"] > 0 and calls["wgrad"] > 0, calls

    assert set(g32) == set(glib) == set(ghip) and len(g32) > 50

    def rel(g, name):
        return ((g[name] - g32[name]).norm() / (g32[name].norm() + 1e-30)).item()

    failures = []
    for name in g32:
        assert torch.isfinite(ghip[name]).all(), name
        assert torch.isfinite(glib[name]).all(), name
        e_hip, e_lib = rel(ghip, name), rel(glib, name)
        print(f"{name:48s} err_hip {e_hip:.4e}  err_lib {e_lib:.4e}")
        if not e_hip <= 2 * e_lib + 1e-3:
            failures.append((name, e_hip, e_lib))
    assert not failures, failures
