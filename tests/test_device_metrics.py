"""Loss and accuracy on the device: the ``k_ce_metrics`` kernel, its binding
and autograd Function, ``train.DeviceMetrics`` and the ``Model.fit`` /
``evaluate`` path that reads metrics back once per epoch.

Kernel tolerances are those of ``tests/test_kernels.py::test_softmax_ce_parity``
(loss atol = rtol = 1e-4; fp32 gradient atol 1e-5, rtol 1e-4) against
``F.cross_entropy`` on the widened logits. A bf16 gradient is the fp32 one
rounded once more: ``|g - bf16(g_ref)| <= ulp_bf16(g_ref) + 1e-5``.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from ddlw_amd.models import build_model

ENV_SWITCHES = ("DDLW_DISABLE_HIP_OPS", "DDLW_EVAL_FOLD", "DDLW_CONV",
                "DDLW_STEM_U8", "DDLW_PW_TRAIN")
BS = (1, 3, 5, 64, 67)             # rows: not a multiple of the waves per block
KS = (1, 5, 33, 64, 65, 1000)      # one class, the workload, around a wave, the bench
DTYPES = (torch.float32, torch.bfloat16)


def _dev():
    return torch.device("cuda:0")


def _clear_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


# --------------------------------------------------------------------------- #
# kernel
# --------------------------------------------------------------------------- #


@functools.lru_cache(maxsize=None)
def _case(B, K, dtype, scale=4.0, seed=11):
    """Logits, labels and the torch reference of one shape, built once (on
    the host, so the reference does not depend on the device) and shared.
    Row 0 is all ties with label 0: torch's argmax picks index 0."""
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * B + K)
    logits = (torch.randn(B, K, generator=g) * scale).to(dtype)
    labels = torch.randint(0, K, (B,), generator=g)
    logits[0] = 0
    labels[0] = 0
    ref_in = logits.float().clone().requires_grad_(True)
    loss = F.cross_entropy(ref_in, labels)
    loss.backward()
    acc = (logits.float().argmax(-1) == labels).float().mean()
    return logits, labels, loss.detach(), ref_in.grad, acc


def _ulp_bf16(x):
    """Spacing of bf16 (8 significant bits) at |x|; 0 at 0."""
    _, e = torch.frexp(x.abs())  # |x| = m * 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def _check(B, K, dtype, scale=4.0):
    from ddlw_amd.ops import binding

    logits, labels, loss_ref, g_ref, acc_ref = _case(B, K, dtype, scale)
    step_out, dlogits = binding.ce_metrics(logits.to(_dev()), labels.to(_dev()), 1.0 / B)
    step_out, g = step_out.cpu(), dlogits.cpu()
    assert dlogits.dtype == dtype and g.shape == (B, K)
    what = f"B={B} K={K} {dtype} scale={scale}"
    print(f"{what}: loss {step_out[0].item():.6f} ref {loss_ref.item():.6f} "
          f"acc {step_out[1].item():.6f} ref {acc_ref.item():.6f} "
          f"max |dg| {(g.float() - g_ref).abs().max().item():.3e}")
    assert torch.allclose(step_out[0], loss_ref, atol=1e-4, rtol=1e-4), what
    assert step_out[1].item() == acc_ref.item(), what
    if dtype == torch.float32:
        assert torch.allclose(g, g_ref, atol=1e-5, rtol=1e-4), what
    else:
        err = (g.float() - g_ref.to(torch.bfloat16).float()).abs()
        assert bool((err <= _ulp_bf16(g_ref) + 1e-5).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("K", KS)
def test_ce_metrics_parity(K, dtype):
    for B in BS:
        _check(B, K, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_ce_metrics_large_logits(dtype):
    """Logits of +-1e4: exp() of them overflows unless the row maximum is
    subtracted first."""
    _check(64, 33, dtype, scale=2500.0)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (49, 67))
def test_ce_metrics_accuracy_is_the_rounded_quotient(B):
    """correct / B for every count: a multiply by 1 / B is off by an ulp for
    some of them (49 * (1 / 49) < 1)."""
    from ddlw_amd.ops import binding

    logits = torch.zeros(B, 5, device=_dev())
    logits[:, 2] = 1.0
    outs = []
    for c in range(B + 1):
        labels = torch.full((B,), 3, device=_dev())
        labels[:c] = 2
        outs.append(binding.ce_metrics(logits, labels, 1.0 / B, want_grad=False)[0])
    got = torch.stack(outs)[:, 1].cpu()
    want = torch.arange(B + 1, dtype=torch.float32) / B
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_ce_metrics_both_launch_regimes():
    from ddlw_amd.ops import binding

    assert binding.ce_metrics_nblocks(64, 5) == 1
    assert binding.ce_metrics_nblocks(256, 1000) == 1
    # rows kernel + finalize: one row per wave, and the capped grid-stride walk
    assert 1 < binding.ce_metrics_nblocks(300, 1000) < 256
    assert binding.ce_metrics_nblocks(70001, 5) == 256
    for dtype in DTYPES:
        _check(256, 1000, dtype)
        _check(300, 1000, dtype)
        _check(70001, 5, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_ce_metrics_is_deterministic(dtype):
    from ddlw_amd.ops import binding

    for B, K in ((67, 1000), (300, 1000), (70001, 5)):
        logits, labels = (t.to(_dev()) for t in _case(B, K, dtype)[:2])
        s1, g1 = binding.ce_metrics(logits, labels, 1.0 / B)
        s2, g2 = binding.ce_metrics(logits, labels, 1.0 / B)
        assert torch.equal(s1, s2) and torch.equal(g1, g2), (B, K)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_ce_metrics_bad_labels(dtype):
    """Labels -1 and K in middle rows (even an unchecked read stays inside
    the tensor): no loss, no gradient, wrong, counted, reported."""
    from ddlw_amd.ops import binding
    from ddlw_amd.train.metrics import DeviceMetrics

    B, K = 16, 5
    logits, labels = _case(B, K, dtype)[:2]
    labels = labels.clone()
    labels[5], labels[9] = -1, K
    ok = (labels >= 0) & (labels < K)
    rows = F.cross_entropy(logits.float()[ok], labels[ok], reduction="none")
    loss_ref = rows.sum() / B
    acc_ref = ((logits.float().argmax(-1) == labels) & ok).sum().float() / B

    accum = torch.zeros(4, dtype=torch.float64, device=_dev())
    step_out, g = binding.ce_metrics(logits.to(_dev()), labels.to(_dev()), 1.0 / B, accum)
    step_out, g = step_out.cpu(), g.cpu()
    assert torch.equal(g[5], torch.zeros(K, dtype=dtype))
    assert torch.equal(g[9], torch.zeros(K, dtype=dtype))
    assert bool((g[ok].float().abs().sum(-1) > 0).all())
    assert torch.allclose(step_out[0], loss_ref, atol=1e-4, rtol=1e-4)
    assert step_out[1].item() == acc_ref.item()
    assert accum.tolist()[2:] == [1.0, 2.0]

    dm = DeviceMetrics(_dev())
    dm.update(logits.to(_dev()), labels.to(_dev()))
    with pytest.raises(ValueError, match="2 label"):
        dm.result()


@pytest.mark.gpu
def test_device_metrics_accumulator(monkeypatch):
    """accum holds the double sums of the fp32 step values, as the host loop
    ``agg[k] += float(v)`` would."""
    from ddlw_amd.ops import binding
    from ddlw_amd.train.metrics import DeviceMetrics

    _clear_env(monkeypatch)
    dm = DeviceMetrics(_dev())
    assert dm.result() == {}
    loss_sum = acc_sum = 0.0
    for B in (8, 5, 64):
        logits, labels = (t.to(_dev()) for t in _case(B, 5, torch.bfloat16)[:2])
        loss = dm.update(logits, labels)
        step = dm.step_out.tolist()
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.item() == step[0]
        loss_sum += step[0]
        acc_sum += step[1]
    assert dm.accum.tolist() == [loss_sum, acc_sum, 3.0, 0.0]
    assert dm.result() == {"loss": loss_sum / 3, "accuracy": acc_sum / 3}
    assert dm.result(()) == {"loss": loss_sum / 3}
    dm.reset()
    assert dm.accum.tolist() == [0.0] * 4 and dm.result() == {}

    step_out, g = binding.ce_metrics(logits, labels, 1.0 / 64, want_grad=False)
    assert g is None and step_out.tolist() == step
    with pytest.raises(TypeError, match="bf16 or fp32"):
        binding.ce_metrics(logits.half(), labels, 1.0 / 64)
    # int32 labels are cast
    s32, _ = binding.ce_metrics(logits, labels.int(), 1.0 / 64, want_grad=False)
    assert s32.tolist() == step


@pytest.mark.gpu
def test_softmax_ce_metrics_gradient_dtype_and_reach(monkeypatch):
    from ddlw_amd.ops import binding, softmax_ce_metrics

    _clear_env(monkeypatch)
    B, K = 64, 5
    logits, labels = (t.to(_dev()) for t in _case(B, K, torch.bfloat16)[:2])
    x = logits.clone().requires_grad_(True)
    loss, step_out = softmax_ce_metrics(x, labels)
    assert loss.requires_grad and not step_out.requires_grad
    (2 * loss).backward()
    assert x.grad.dtype == torch.bfloat16
    _, g = binding.ce_metrics(logits, labels, 1.0 / B)
    assert torch.equal(x.grad, g * 2) and bool(g.float().abs().sum() > 0)

    # the torch-op path computes the same values, accumulators included
    monkeypatch.setenv("DDLW_DISABLE_HIP_OPS", "1")
    accum = torch.zeros(4, dtype=torch.float64, device=_dev())
    x2 = logits.clone().requires_grad_(True)
    loss2, step2 = softmax_ce_metrics(x2, labels, accum)
    loss2.backward()
    assert torch.allclose(step2[0], step_out[0], atol=1e-4, rtol=1e-4)
    assert step2[1].item() == step_out[1].item()
    assert x2.grad.dtype == torch.bfloat16
    assert accum.tolist() == [step2[0].item(), step2[1].item(), 1.0, 0.0]


# --------------------------------------------------------------------------- #
# facade
# --------------------------------------------------------------------------- #


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


def _module(seed=31):
    torch.manual_seed(seed)
    m = build_model(64, 64, 3, 5, dropout=0.0)
    _randomize_bn(m, seed=9)
    return m


def _batches(n, seed=5, batch=8):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randint(0, 256, (batch, 64, 64, 3), dtype=torch.uint8, generator=g),
             torch.randint(0, 5, (batch,), generator=g)) for _ in range(n)]


def _facade(module, lr=None):
    from ddlw_amd.train import Model

    return Model(module, _dev(), precision="bf16").compile("Adam", learning_rate=lr)


@pytest.mark.gpu
def test_fit_history_is_the_mean_of_its_steps(monkeypatch):
    _clear_env(monkeypatch)
    m = _module()
    m2 = copy.deepcopy(m)
    batches = _batches(6)

    hist = _facade(m).fit(batches, epochs=2, steps_per_epoch=3, verbose=0,
                          metrics_on_device=True).history

    hand = _facade(m2)
    it = iter(batches)
    for epoch in range(2):
        loss_sum = acc_sum = 0.0
        for _ in range(3):
            hand.train_step_async(*next(it))
            step = hand.train_metrics.step_out.tolist()
            loss_sum += step[0]
            acc_sum += step[1]
        assert hist["loss"][epoch] == loss_sum / 3
        assert hist["accuracy"][epoch] == acc_sum / 3
    assert set(hist) == {"loss", "accuracy"} and len(hist["loss"]) == 2
    assert hist["loss"][0] != hist["loss"][1]


@pytest.mark.gpu
def test_device_path_equals_per_step_path(monkeypatch):
    """Learning rate 0: the weights cannot move, so both paths see the same
    logits in every step."""
    _clear_env(monkeypatch)
    m = _module()
    m2 = copy.deepcopy(m)
    batches, val = _batches(6), _batches(2, seed=6)
    kw = dict(epochs=2, steps_per_epoch=3, validation_data=val, validation_steps=2,
              verbose=0)
    on = _facade(m, lr=0.0).fit(batches, metrics_on_device=True, **kw).history
    off = _facade(m2, lr=0.0).fit(batches, metrics_on_device=False, **kw).history
    assert set(on) == set(off) == {"loss", "accuracy", "val_loss", "val_accuracy"}
    print("device path", on, "per-step path", off)
    for k in ("accuracy", "val_accuracy"):
        assert on[k] == off[k], k
    for k in ("loss", "val_loss"):
        assert torch.allclose(torch.tensor(on[k]), torch.tensor(off[k]),
                              atol=1e-4, rtol=1e-4), k

    ev_on = _facade(m, lr=0.0).evaluate(val, steps=2, metrics_on_device=True)
    ev_off = _facade(m2, lr=0.0).evaluate(val, steps=2, metrics_on_device=False)
    assert len(ev_on) == len(ev_off) == 2 and ev_on[1] == ev_off[1]
    assert abs(ev_on[0] - ev_off[0]) <= 1e-4 + 1e-4 * abs(ev_off[0])


@pytest.mark.gpu
def test_no_readback_inside_the_step_loop(monkeypatch):
    from ddlw_amd.train import Callback
    from ddlw_amd.train.metrics import DeviceMetrics

    _clear_env(monkeypatch)
    model = _facade(_module())
    batches, val = _batches(6), _batches(2, seed=6)

    reads = {"__float__": 0, "item": 0, "tolist": 0, "cpu": 0}
    for name in reads:
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **k):
            reads[_name] += 1
            return _real(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, counted)

    marks = []  # (what, reads so far)

    class Mark(Callback):
        def on_epoch_begin(self, epoch, logs=None):
            marks.append(("begin", dict(reads)))

    real_result = DeviceMetrics.result

    def result(self, *a, **k):
        which = "train" if self is model.train_metrics else "val"
        marks.append((which + "_result", dict(reads)))
        out = real_result(self, *a, **k)
        marks.append((which + "_done", dict(reads)))
        return out

    monkeypatch.setattr(DeviceMetrics, "result", result)
    monkeypatch.setattr(model, "train_step",
                        lambda *a, **k: pytest.fail("train_step on the device path"))
    monkeypatch.setattr(model, "eval_step",
                        lambda *a, **k: pytest.fail("eval_step on the device path"))

    model.fit(batches, epochs=2, steps_per_epoch=3, validation_data=val,
              validation_steps=2, callbacks=[Mark()], verbose=0, metrics_on_device=True)
    assert [w for w, _ in marks] == ["begin", "train_result", "train_done",
                                     "val_result", "val_done"] * 2
    for e in (0, 5):
        begin, train_result, train_done, val_result, val_done = (r for _, r in marks[e:e + 5])
        assert train_result == begin, (begin, train_result)   # the step loop read nothing
        assert val_result == train_done, (train_done, val_result)
        for a, b in ((train_result, train_done), (val_result, val_done)):
            assert sum(b.values()) - sum(a.values()) == 1     # one copy per result()
    monkeypatch.undo()

    _clear_env(monkeypatch)
    floats = [0]
    real_float = torch.Tensor.__float__

    def counted_float(self):
        floats[0] += 1
        return real_float(self)

    monkeypatch.setattr(torch.Tensor, "__float__", counted_float)
    model.fit(batches, epochs=1, steps_per_epoch=3, verbose=0, metrics_on_device=False)
    assert floats[0] >= 3


@pytest.mark.gpu
def test_fallback_to_the_per_step_path(monkeypatch):
    from ddlw_amd.train import Callback, Model

    _clear_env(monkeypatch)
    seen = []

    class PerBatch(Callback):
        def on_batch_end(self, batch, logs=None):
            seen.append(logs)

    model = _facade(_module())
    batches = _batches(3)
    model.fit(batches, epochs=1, steps_per_epoch=3, callbacks=[PerBatch()], verbose=0)
    assert len(seen) == 3
    for logs in seen:
        assert set(logs) == {"loss", "accuracy"}
        assert all(type(v) is float for v in logs.values())
    with pytest.raises(ValueError, match="on_batch_end"):
        model.fit(batches, epochs=1, steps_per_epoch=3, callbacks=[PerBatch()],
                  verbose=0, metrics_on_device=True)

    # None as shipped is the per-step path everywhere (the device path did
    # not beat it by more than its spread): nothing reaches DeviceMetrics
    from ddlw_amd.train import model as model_mod
    from ddlw_amd.train.metrics import DeviceMetrics

    assert model_mod._DEVICE_METRICS_DEFAULT is False
    plain = _facade(_module())
    plain.fit(batches, epochs=1, steps_per_epoch=3, validation_data=_batches(2, seed=6),
              validation_steps=2, verbose=0)
    assert plain._train_metrics is None and plain._eval_metrics is None

    # auto switched on, the mixed case: the callback holds training on the
    # per-step path, the validation pass has no callbacks and stays on the
    # device
    monkeypatch.setattr(model_mod, "_DEVICE_METRICS_DEFAULT", True)
    results = []
    real_result = DeviceMetrics.result
    monkeypatch.setattr(DeviceMetrics, "result",
                        lambda self, *a, **k: results.append(self) or real_result(self, *a, **k))
    monkeypatch.setattr(model, "eval_step",
                        lambda *a, **k: pytest.fail("eval_step under None"))
    del seen[:]
    hist = model.fit(batches, epochs=1, steps_per_epoch=3, callbacks=[PerBatch()],
                     validation_data=_batches(2, seed=6), validation_steps=2,
                     verbose=0).history
    assert len(seen) == 3 and results == [model.eval_metrics]
    assert set(hist) == {"loss", "accuracy", "val_loss", "val_accuracy"}
    monkeypatch.undo()
    _clear_env(monkeypatch)

    # a loss of the caller's own, and a metric the kernel does not compute
    custom = Model(_module(), _dev(), precision="bf16").compile(
        "Adam", loss=lambda lg, lb: F.cross_entropy(lg.float(), lb))
    hist = custom.fit(batches, epochs=1, steps_per_epoch=3, verbose=0).history
    assert custom._train_metrics is None and len(hist["loss"]) == 1
    with pytest.raises(ValueError, match="loss"):
        custom.fit(batches, epochs=1, steps_per_epoch=3, verbose=0, metrics_on_device=True)
    model.compile("Adam", metrics=("accuracy", "top5"))
    with pytest.raises(ValueError, match="top5"):
        model.evaluate(batches, steps=1, metrics_on_device=True)
    monkeypatch.setenv("DDLW_DISABLE_HIP_OPS", "1")
    with pytest.raises(ValueError, match="DDLW_DISABLE_HIP_OPS"):
        _facade(_module()).evaluate(batches, steps=1, metrics_on_device=True)


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #


def _cpu_model(**compile_kw):
    from ddlw_amd.train import Model

    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 5))
    return Model(net, torch.device("cpu")).compile("SGD", **compile_kw)


def _cpu_batches(n=3):
    g = torch.Generator().manual_seed(4)
    return [(torch.randn(4, 3, 2, 2, generator=g), torch.randint(0, 5, (4,), generator=g))
            for _ in range(n)]


def test_cpu_model_takes_the_per_step_path(monkeypatch):
    model = _cpu_model()
    steps = [0]
    real = model.train_step

    def counted(*a, **k):
        steps[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(model, "train_step", counted)
    hist = model.fit(_cpu_batches(), epochs=1, steps_per_epoch=3, verbose=0).history
    assert steps[0] == 3 and model._train_metrics is None
    assert set(hist) == {"loss", "accuracy"}
    assert model.RUN_AHEAD >= 1
    with pytest.raises(ValueError, match="CUDA"):
        model.fit(_cpu_batches(), epochs=1, steps_per_epoch=3, verbose=0,
                  metrics_on_device=True)
    with pytest.raises(ValueError, match="CUDA"):
        model.evaluate(_cpu_batches(), steps=1, metrics_on_device=True)
    assert len(model.evaluate(_cpu_batches(), steps=2)) == 2


def test_custom_loss_falls_back(monkeypatch):
    model = _cpu_model(loss=lambda lg, lb: F.cross_entropy(lg, lb))
    hist = model.fit(_cpu_batches(), epochs=1, steps_per_epoch=3, verbose=0).history
    assert len(hist["loss"]) == 1 and model._train_metrics is None
    with pytest.raises(ValueError):
        model.fit(_cpu_batches(), epochs=1, steps_per_epoch=3, verbose=0,
                  metrics_on_device=True)
    # the loss is a reason of its own where the device and the library are not
    import ddlw_amd.ops as ops

    monkeypatch.delenv("DDLW_DISABLE_HIP_OPS", raising=False)
    monkeypatch.setattr(model, "device", torch.device("cuda:0"))
    monkeypatch.setattr(ops, "has_lib", lambda: True)
    why = model._device_metrics_blocker(())
    assert why is not None and "loss" in why
    model.loss_fn = _cpu_model().loss_fn
    assert model._device_metrics_blocker(()) is None


def test_device_metrics_on_cpu_matches_torch():
    from ddlw_amd.train.metrics import DeviceMetrics

    dm = DeviceMetrics("cpu")
    assert dm.result() == {}
    losses, accs = [], []
    for B in (8, 5, 3):
        logits, labels, loss_ref, g_ref, acc_ref = _case(B, 5, torch.float32)
        x = logits.clone().requires_grad_(True)
        loss = dm.update(x, labels)
        loss.backward()
        assert torch.allclose(loss.detach(), loss_ref, atol=1e-4, rtol=1e-4)
        assert torch.allclose(x.grad, g_ref, atol=1e-5, rtol=1e-4)
        assert dm.step_out[1].item() == acc_ref.item()
        losses.append(dm.step_out[0].item())
        accs.append(acc_ref.item())
    out = dm.result()
    assert out == {"loss": sum(losses) / 3, "accuracy": sum(accs) / 3}
    assert dm.accum.tolist()[2:] == [3.0, 0.0]

    labels = labels.clone()
    labels[1] = 7
    dm.update(logits, labels)
    with pytest.raises(ValueError, match="1 label"):
        dm.result()
    dm.reset()
    assert dm.result() == {}
