"""Dropout + dense in one kernel each way (``hip/head_dense.hip``): routing,
the kernels against fp64, and ``TransferModel`` with ``DDLW_HEAD_DENSE`` 1
against 0.

Reference: fp64 products of the bf16 operands, with ``yd`` the dropped
activations of the existing ``dropout_fwd`` (so the mask rule is pinned to it)
and ``dl16`` the dlogits rounded to bf16. bf16 products are exact in fp32, so
only the fp32 sum over the reduction (depth D: D * 2^-23 of the sum of
magnitudes) and the one rounding to bf16 (2^-8 relative) contribute.
"""
import copy

import pytest
import torch

R, E = 2.0 ** -8, 2.0 ** -23


@pytest.mark.parametrize("mode, C, K, N, want", [
    ("0", 1280, 5, 64, False), ("1", 1280, 5, 64, True), ("1", 8, 64, 1, True),
    ("1", 1280, 65, 64, False), ("1", 1284, 5, 64, False), ("1", 1280, 5, 0, False),
    (None, 1280, 65, 64, False), (None, 1280, 5, 64, None)])
def test_route(monkeypatch, mode, C, K, N, want):
    from ddlw_amd.ops import binding

    monkeypatch.delenv("DDLW_HEAD_DENSE", raising=False)
    if mode is not None:
        monkeypatch.setenv("DDLW_HEAD_DENSE", mode)
    if want is None:  # unset: the measured table decides
        row = binding._HEAD_DENSE_MEASURED.get((C, K))
        want = row is not None and row[0] <= N <= row[1]
    assert binding.head_dense_route(C, K, N) is want


@pytest.mark.parametrize("train", [False, True])
def test_cpu_model_is_unchanged(monkeypatch, train):
    from ddlw_amd.models import build_model
    from ddlw_amd.ops import binding

    def never(*a, **k):
        raise AssertionError("the kernel path was taken on CPU")

    monkeypatch.setattr(binding, "head_dense_fwd", never)
    m = build_model(32, 32, 3, 5).train(train)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DDLW_HEAD_DENSE", mode)
        torch.manual_seed(7)  # the stock dropout draws from torch's generator
        out[mode] = m(x)
    assert out["1"].dtype == torch.float32 and torch.equal(out["0"], out["1"])


def _within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    print(f"{what}: max err / bound = {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), what


# N, C, K, p, bias, fp32 dlogits, dx wanted
CASES = [(17, 40, 17, 0.5, True, False, True), (1, 8, 1, 0.5, False, True, False),
         (64, 1280, 5, 0.5, True, False, True), (64, 1280, 5, 0.0, True, True, False),
         (17, 1280, 64, 0.5, False, True, True), (64, 40, 16, 0.0, False, False, True),
         (1, 8, 64, 0.5, True, False, True), (17, 8, 5, 0.5, True, True, False),
         (40, 72, 33, 0.5, True, False, True)]  # a batch-step tail, a column-tile tail


@pytest.mark.gpu
@pytest.mark.parametrize("N, C, K, p, bias, f32, want_dx", CASES)
def test_kernels_against_fp64(N, C, K, p, bias, f32, want_dx):
    from ddlw_amd.ops import binding

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(N * 131 + C * 7 + K)
    x = torch.randn(N, C, generator=g).to(torch.bfloat16).to(dev)
    w = (0.05 * torch.randn(K, C, generator=g)).to(torch.bfloat16).to(dev)
    b = (0.05 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev) if bias else None
    dl = (torch.randn(N, K, generator=g) / N).to(dev)
    dl = dl if f32 else dl.to(torch.bfloat16)
    seed, scale = 0x1234567 + N, 1.0 / (1.0 - p)
    if p > 0:
        yd, mb = binding.dropout_fwd(x, p, seed)
        mask = ((mb.view(N, C // 8, 1) >> torch.arange(8, device=dev)) & 1).view(N, C).double()
    else:
        yd, mask = x, torch.ones(N, C, dtype=torch.float64, device=dev)
    yd, wd, dl16 = yd.double(), w.double(), dl.to(torch.bfloat16).double()
    bd = b.double() if bias else torch.zeros(K, dtype=torch.float64, device=dev)
    what = f"N{N} C{C} K{K} p{p}"

    y = binding.head_dense_fwd(x, w, b, p, seed)
    ref = yd @ wd.t() + bd
    _within(y, ref, R * ref.abs() + C * E * (yd.abs() @ wd.abs().t() + bd.abs()), what + " logits")
    assert torch.equal(y, binding.head_dense_fwd(x, w, b, p, seed))

    dW, db, dx = binding.head_dense_bwd(dl, x, w, p, seed, want_dx, bias)
    again = binding.head_dense_bwd(dl, x, w, p, seed, want_dx, bias)
    refW = dl16.t() @ yd
    _within(dW, refW, R * refW.abs() + N * E * (dl16.abs().t() @ yd.abs()), what + " dW")
    assert torch.equal(dW, again[0])
    assert (db is None) == (not bias) and (dx is None) == (not want_dx)
    if bias:
        refb = dl16.sum(0)
        _within(db, refb, R * refb.abs() + N * E * dl16.abs().sum(0), what + " db")
        assert torch.equal(db, again[1])
    if want_dx:
        refx = mask * scale * (dl16 @ wd)
        _within(dx, refx, R * refx.abs() + K * E * scale * (dl16.abs() @ wd.abs()), what + " dx")
        assert (dx[mask == 0] == 0).all() and torch.equal(dx, again[2])


def _step(model, mode, train, u8, labels, monkeypatch, env=()):
    """Forward (+ loss and backward in training) of a copy of ``model`` under
    ``DDLW_HEAD_DENSE=mode``: the copy, its logits and the logits' gradient."""
    from ddlw_amd.ops.layers import softmax_cross_entropy

    monkeypatch.setenv("DDLW_HEAD_DENSE", mode)
    for k, v in env:
        monkeypatch.setenv(k, v)
    m = copy.deepcopy(model).train(train)
    dl = []
    with torch.set_grad_enabled(train):
        logits = m(u8)
        if train:
            logits.register_hook(dl.append)
            softmax_cross_entropy(logits, labels).backward()
    for k, _ in env:
        monkeypatch.delenv(k)
    return m, logits.detach(), (dl[0] if dl else None)


@pytest.mark.gpu
@pytest.mark.parametrize("train", [True, False])
def test_model_agrees_with_the_unfused_head(monkeypatch, train):
    """Logits and the classifier's gradients of the two paths within twice the
    kernel bounds (both round the same exact value once); the same dropout
    seed on both sides, or the training logits would differ grossly."""
    from ddlw_amd.models import build_model
    from ddlw_amd.ops import apply_bf16_policy, binding

    torch.manual_seed(5)
    model = apply_bf16_policy(build_model(32, 32, 3, 5).to("cuda:0"))
    u8 = torch.randint(0, 256, (9, 32, 32, 3), dtype=torch.uint8).to("cuda:0").permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (9,)).to("cuda:0")
    calls = []
    real = binding.head_dense_fwd
    monkeypatch.setattr(binding, "head_dense_fwd", lambda *a: (calls.append(a[3]), real(*a))[1])
    m0, y0, _ = _step(model, "0", train, u8, labels, monkeypatch)
    assert not calls
    m1, y1, dl = _step(model, "1", train, u8, labels, monkeypatch)
    assert calls == [0.5 if train else 0.0] and m0.dropout._calls == m1.dropout._calls == int(train)

    with torch.no_grad():
        x = m1.base(u8, pooled=True)
    yd = binding.dropout_fwd(x, 0.5, m1.dropout._base_seed + 0x9E3779B97F4A7C15)[0] if train else x
    yd, wd, bd = yd.double(), m1.classifier.weight.double(), m1.classifier.bias.double()
    N, C = yd.shape
    ref = yd @ wd.t() + bd
    _within(y1, y0.double(), 2 * (R * ref.abs() + C * E * (yd.abs() @ wd.abs().t() + bd.abs())),
            "model logits")
    if train:
        dl16 = dl.to(torch.bfloat16).double()
        refW, refb = dl16.t() @ yd, dl16.sum(0)
        _within(m1.classifier.weight.grad, m0.classifier.weight.grad.double(),
                2 * (R * refW.abs() + N * E * (dl16.abs().t() @ yd.abs())), "model dW")
        _within(m1.classifier.bias.grad, m0.classifier.bias.grad.double(),
                2 * (R * refb.abs() + N * E * dl16.abs().sum(0)), "model db")


@pytest.mark.gpu
def test_dx_reaches_the_trainable_tail(monkeypatch):
    """``fine_tune_at=20``: dx flows into the 320 -> 1280 conv. Its gradient
    by the rule of ``test_finetune.py``: relative L2 error to the fp32 stock
    model at most twice that of the unfused bf16 path plus 1e-3. dropout=0, so
    that the fp32 model (another generator) sees the same activations; dx
    under a mask is checked against fp64 above."""
    from ddlw_amd.models import build_model
    from ddlw_amd.ops import apply_bf16_policy

    torch.manual_seed(6)
    m32 = build_model(32, 32, 3, 5, dropout=0.0, fine_tune_at=20).to("cuda:0")
    u8 = torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8).to("cuda:0").permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (8,)).to("cuda:0")
    m16 = apply_bf16_policy(copy.deepcopy(m32))
    grad = {"32": _step(m32, "0", True, u8, labels, monkeypatch,
                        env=(("DDLW_DISABLE_HIP_OPS", "1"),))[0]}
    grad["0"] = _step(m16, "0", True, u8, labels, monkeypatch)[0]
    grad["1"] = _step(m16, "1", True, u8, labels, monkeypatch)[0]
    g = {k: m.base.base.features[20].weight.grad.double() for k, m in grad.items()}
    err = {k: ((g[k] - g["32"]).norm() / g["32"].norm()).item() for k in ("0", "1")}
    print(f"features[20].weight.grad: err fused {err['1']:.4e}, unfused {err['0']:.4e}")
    assert torch.isfinite(g["1"]).all() and err["1"] <= 2 * err["0"] + 1e-3
