"""Depthwise conv + BatchNorm training stage: ``depthwise_fwd_stats``,
``depthwise_bwd_bn``, the stage Function and the routing under
``DDLW_DW_TRAIN``. Bounds: the conv bound of test_depthwise_bwd.py, the
statistics rule and the two-pipeline rule of test_pw_train.py.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from ddlw_amd.models.mobilenet_v2 import InvertedResidual
from ddlw_amd.ops import mbconv
from ddlw_amd.ops.conv import Conv2d
from ddlw_amd.ops.layers import BatchNormAct2d
from test_pw_train import (_assert_regions, _assert_two_pipelines, _bf16_randn,  # the
                           _block_step, _count_calls, _dev, _rel_l2,  # project's helpers
                           _stat_errors, _to_bf16_convs)

BOUND = 5e-2
EPS, MOM = 1e-5, 0.1
ENV_SWITCHES = ("DDLW_DISABLE_HIP_OPS", "DDLW_EVAL_FOLD", "DDLW_CONV", "DDLW_PW_TRAIN",
                "DDLW_DW_TRAIN")
NEW_FUNCTIONS = ("depthwise_fwd_stats", "depthwise_bwd_bn")

# (N, H, W, C, stride), pad 1, 3x3
SHAPES = [
    (3, 20, 20, 96, 1),   # baseline
    (2, 15, 17, 24, 1),   # non-square, tile tails on both axes, vecC = 3
    (1, 2, 2, 960, 1),    # every tap pads, the tile is all halo
    (1, 1, 1, 8, 1),      # single vector, single pixel
    (4, 28, 28, 32, 1),   # many tiles per persistent block, many partials
    (1, 3, 3, 2056, 1),   # vecC = 257: a partly idle channel-group column
    (2, 15, 15, 24, 2),   # stride 2, forward kernel only
    (2, 7, 7, 576, 2),    # stride 2, forward kernel only
]
S1_SHAPES = [s for s in SHAPES if s[4] == 1]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """CPU, computed once and shared: bf16-rounded inputs and fp64 autograd
    through conv -> batch norm (-> hardtanh(0, 6) under ``relu``). The batch
    norm is written out: ``F.batch_norm`` refuses one value per channel.
    beta cycles through -3, 1, 5, 9 and gamma is ~3, so every ReLU6 region
    is well filled at any row count; dout has mean 0.5, so D is far from 0."""
    n, h, w, c, st = shape
    g = torch.Generator(device="cpu").manual_seed(2000 + sum(shape))
    x = _bf16_randn(n, c, h, w, g=g)
    wt = _bf16_randn(c, 1, 3, 3, g=g)
    ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
    dout = (torch.randn(n, c, ho, wo, generator=g) + 0.5).to(torch.bfloat16)
    gamma = torch.empty(c).uniform_(0.9, 1.1, generator=g) * 3.0
    beta = (torch.arange(c) % 4).float() * 4.0 - 3.0
    ref = {"y": F.conv2d(x.float(), wt.float(), stride=st, padding=1, groups=c)}
    for relu in (False, True):
        x64 = x.double().requires_grad_(True)
        w64 = wt.double().requires_grad_(True)
        z = F.conv2d(x64, w64, stride=st, padding=1, groups=c)
        mean = z.mean((0, 2, 3), keepdim=True)
        var = ((z - mean) ** 2).mean((0, 2, 3), keepdim=True)
        pre = ((z - mean) / (var + EPS).sqrt() * gamma.double().view(1, c, 1, 1)
               + beta.double().view(1, c, 1, 1))
        out = F.hardtanh(pre, 0.0, 6.0) if relu else pre
        (out * dout.double()).sum().backward()
        ref[relu] = (x64.grad, w64.grad, pre.detach())
    return x, wt, dout, gamma, beta, ref


@pytest.mark.parametrize("shape", S1_SHAPES)
def test_case_inputs_cover_relu6_regions(shape):
    """CPU, the reference alone: the inputs of the backward test put >= 5% of
    the pre-activation into each ReLU6 region."""
    _assert_regions(_case(shape)[5][True][2], f"dw stage {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_depthwise_fwd_stats(shape):
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import query

    n, h, w, c, st = shape
    dev = _dev()
    x, wt, _, _, _, ref = _case(shape)
    x, wt = _cl(x.to(dev)), wt.to(dev)
    ho, wo = ref["y"].shape[2:]
    rows = n * ho * wo
    g = torch.Generator(device="cpu").manual_seed(c + rows)
    rm0 = torch.empty(c).uniform_(-0.3, 0.3, generator=g).to(dev)
    rv0 = torch.empty(c).uniform_(0.5, 1.5, generator=g).to(dev)

    nparts_q = int(query("depthwise_fwd_stats_nparts", rows, c, None))
    assert 1 <= nparts_q <= 512
    PAD = 2
    buf = torch.full((2, nparts_q + 2 * PAD, c), -1234.0, dtype=torch.float32, device=dev)
    before = buf.clone()
    parts = (buf[0, PAD:PAD + nparts_q], buf[1, PAD:PAD + nparts_q])
    y, ps, pq, nparts = binding.depthwise_fwd_stats(x, wt, st, 1, parts=parts)
    assert nparts == nparts_q
    assert ps.data_ptr() == parts[0].data_ptr() and pq.data_ptr() == parts[1].data_ptr()
    assert y.shape == ref["y"].shape and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(buf[:, :PAD], before[:, :PAD])
    assert torch.equal(buf[:, PAD + nparts:], before[:, PAD + nparts:])
    err = ((y.float().cpu() - ref["y"]).abs().max() / (ref["y"].abs().max() + 1e-6)).item()
    print(f"fwd_stats {shape}: rel err {err:.3e}")
    assert err < BOUND, (shape, err)

    y2, ps2, pq2, _ = binding.depthwise_fwd_stats(x, wt, st, 1)
    assert torch.equal(y, y2) and torch.equal(ps, ps2) and torch.equal(pq, pq2)

    rm_f, rv_f, rm_s, rv_s = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    mean_f, rstd_f = binding.bn_finalize_parts(ps, pq, nparts, rows, c, EPS, MOM, rm_f, rv_f)
    mean_s, rstd_s = binding.bn_stats(y, EPS, MOM, rm_s, rv_s)
    y64 = y.double().permute(0, 2, 3, 1).reshape(rows, c)
    mean64 = y64.mean(0)
    var64 = ((y64 - mean64) ** 2).mean(0)
    ref64 = (mean64, var64 + EPS, (1 - MOM) * rm0.double() + MOM * mean64,
             (1 - MOM) * rv0.double() + MOM * var64 * rows / max(rows - 1, 1))
    e_f = _stat_errors(mean_f, rstd_f, rm_f, rv_f, ref64)
    e_s = _stat_errors(mean_s, rstd_s, rm_s, rv_s, ref64)
    slack = rows * 2.0 ** -24
    print(f"stats {shape}: fused {e_f}  standalone {e_s}  slack {slack:.3e}")
    for name in e_f:
        assert e_f[name] <= 2 * e_s[name] + slack, (name, e_f[name], e_s[name])


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu6"])
@pytest.mark.parametrize("shape", S1_SHAPES)
def test_depthwise_bwd_bn(shape, relu):
    """Against the unfused route (bn_bwd_dx -> dgrad / wgrad), both measured
    against fp64 autograd through the stage."""
    from ddlw_amd.ops import binding

    n, h, w, c, _ = shape
    dev = _dev()
    x, wt, dout, gamma, beta, ref = _case(shape)
    ref_dx, ref_dw, pre = ref[relu]
    if relu:
        _assert_regions(pre, f"dw stage {shape}")
    x, wt, dout = _cl(x.to(dev)), wt.to(dev), _cl(dout.to(dev))
    gamma, beta = gamma.to(dev), beta.to(dev)
    y = _cl(ref["y"].to(dev).to(torch.bfloat16))
    mean, rstd = binding.bn_stats(y, EPS, MOM, None, None)
    _, mask = binding.bn_apply(y, None, mean, rstd, gamma, beta, 2 if relu else 0)
    dbeta, dgamma = binding.bn_bwd_reduce(dout, mask, y, mean, rstd, relu)
    A = gamma * rstd
    D = A * rstd * dgamma / (n * h * w) * mean - A * dbeta / (n * h * w)

    args = (dout, mask, y, x, wt, mean, rstd, gamma, dbeta, dgamma, relu)
    dx, dw = binding.depthwise_bwd_bn(*args, True)
    assert dx.shape == x.shape and dx.is_contiguous(memory_format=torch.channels_last)
    assert dw.shape == wt.shape and dw.dtype == torch.float32
    dz, _ = binding.bn_bwd_dx(dout, mask, y, mean, rstd, gamma, dbeta, dgamma, relu, False)
    # a halo filled with D instead of 0 would show: D is above bf16's step at max|dz|
    assert D.abs().max().item() > 2.0 ** -7 * dz.float().abs().max().item()
    dx_p = binding.depthwise_dgrad(dz, wt, tuple(x.shape), 1, 1)
    dw_p = binding.depthwise_wgrad(dz, x, tuple(wt.shape), 1, 1)
    what = f"bwd_bn {shape} relu={relu}"
    _assert_two_pipelines(dx.cpu(), dx_p.cpu(), ref_dx, what + " dx")
    _assert_two_pipelines(dw.cpu(), dw_p.cpu(), ref_dw, what + " dw")
    border = torch.zeros(h, w, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    _assert_two_pipelines(dx.cpu()[:, :, border], dx_p.cpu()[:, :, border],
                          ref_dx[:, :, border], what + " dx border")

    none, dw_only = binding.depthwise_bwd_bn(*args, False)
    assert none is None and torch.equal(dw_only, dw)
    dx2, dw2 = binding.depthwise_bwd_bn(*args, True)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)


def _stage_run(conv, bn, x, gout, fused):
    x = _cl(x.detach().clone()).requires_grad_(True)
    y = mbconv.dw_conv_bn_train(conv, bn, x) if fused else bn(conv(x))
    (y.float() * gout.float()).sum().backward()
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": x.grad, "dW": conv.weight.grad,
            "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean.detach().clone(),
            "running_var": bn.running_var.detach().clone(),
            "num_batches_tracked": int(bn.num_batches_tracked)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(24, 1), (96, 2)], ids=lambda c: "c%d_s%d" % c)
def test_stage_function_vs_module_path(case, monkeypatch):
    """One step three ways: fp32 stock ops, bf16 modules, bf16 stage Function."""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    C, st = case
    dev = _dev()
    x, wt, dout, gamma, beta, _ = _case((2, 9, 9, C, st))
    conv32 = Conv2d(C, C, 3, st, 1, groups=C, bias=False).to(dev).train()
    bn32 = BatchNormAct2d(C, act="relu6").to(dev).train()
    with torch.no_grad():
        conv32.weight.copy_(wt.float())
        bn32.weight.copy_(gamma)
        bn32.bias.copy_(beta)
        bn32.running_mean.uniform_(-0.3, 0.3)
        bn32.running_var.uniform_(0.5, 1.5)
    convb, bnb = copy.deepcopy(conv32).to(torch.bfloat16), copy.deepcopy(bn32)
    convn, bnn = copy.deepcopy(convb), copy.deepcopy(bn32)
    x, dout = x.to(dev), dout.to(dev)

    monkeypatch.setenv("DDLW_DISABLE_HIP_OPS", "1")
    ref = _stage_run(conv32, bn32, x.float(), dout.float(), fused=False)
    monkeypatch.delenv("DDLW_DISABLE_HIP_OPS")
    calls = _count_calls(monkeypatch, NEW_FUNCTIONS)
    parent = _stage_run(convb, bnb, x, dout, fused=False)
    assert not any(calls.values()), calls
    new = _stage_run(convn, bnn, x, dout, fused=True)
    assert calls == {"depthwise_fwd_stats": 1, "depthwise_bwd_bn": 1 if st == 1 else 0}, calls

    for name in ("y", "dx", "dW", "dgamma", "dbeta", "running_mean", "running_var"):
        assert new[name].shape == ref[name].shape, name
        _assert_two_pipelines(new[name], parent[name], ref[name], f"dw stage {case} {name}")
    assert new["num_batches_tracked"] == parent["num_batches_tracked"] == 1
    assert new["y"].max().item() == 6.0 and new["y"].min().item() == 0.0


@pytest.mark.gpu
def test_training_block_routing(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    dev = _dev()
    torch.manual_seed(41)
    g = torch.Generator(device="cpu").manual_seed(48)
    x = _cl(_bf16_randn(2, 24, 9, 9, g=g).to(dev))
    blk = _to_bf16_convs(InvertedResidual(24, 24, 1, 6).to(dev)).train()
    blk2 = _to_bf16_convs(InvertedResidual(24, 24, 2, 6).to(dev)).train()
    calls = _count_calls(monkeypatch, NEW_FUNCTIONS + ("bn_stats",))

    def step(module, inp, env):
        calls.update(dict.fromkeys(calls, 0))
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        out = _block_step(module, inp)
        for name in env:
            monkeypatch.delenv(name)
        return out

    y_off, dx_off = step(blk, x, {})                  # the default is off
    assert calls == {"depthwise_fwd_stats": 0, "depthwise_bwd_bn": 0, "bn_stats": 1}, calls
    y_on, dx_on = step(blk, x, {"DDLW_DW_TRAIN": "1"})
    assert calls == {"depthwise_fwd_stats": 1, "depthwise_bwd_bn": 1, "bn_stats": 0}, calls
    assert y_on.shape == y_off.shape and dx_on.shape == dx_off.shape
    assert torch.isfinite(y_on.float()).all() and torch.isfinite(dx_on.float()).all()
    for p in blk.parameters():
        assert p.grad is not None and torch.isfinite(p.grad.float()).all()
    step(blk2, x, {"DDLW_DW_TRAIN": "1"})             # stride 2: forward only
    assert calls["depthwise_fwd_stats"] == 1 and calls["depthwise_bwd_bn"] == 0, calls
    # stock BatchNorm takes no bf16 input: off the gate, step the conv alone
    dw_conv, x144 = mbconv._stages(blk)[1][0], _cl(_bf16_randn(2, 144, 9, 9, g=g).to(dev))
    for module, inp, env, gate in ((blk, x, {"DDLW_DW_TRAIN": "0"}, True),
                                   (blk, x, {"DDLW_CONV": "stock"}, False),
                                   (dw_conv, x144, {"DDLW_DISABLE_HIP_OPS": "1"}, False)):
        step(module, inp, {"DDLW_DW_TRAIN": "1", **env})
        assert not calls["depthwise_fwd_stats"] and not calls["depthwise_bwd_bn"], (env, calls)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        assert mbconv.inverted_residual_train_fusable(blk, x) == gate, env
        for name in env:
            monkeypatch.delenv(name)
