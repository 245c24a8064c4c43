#!/usr/bin/env python3
"""Frozen-MobileNetV2 benchmark: the fused pointwise / depthwise kernels vs
the unfused path (library conv or ``depthwise_fwd``, then the
``BatchNormAct2d`` eval forward, then the eager residual add where the block
has one), per layer and end to end.

Method of ``bench_depthwise.py``: one process, the two contenders alternate
round by round, device events around ``--iters`` back-to-back calls, median
over ``--rounds`` rounds. ``spread`` is max - min of the unfused contender's
rounds. Routing rule (docs/KERNELS.md): a shape stays on the fused kernel
only if its median beats the unfused median by more than that spread;
``keep`` in each record says so.

End to end, fused on vs ``DDLW_EVAL_FOLD=0`` (read at call time):
  - frozen ``MobileNetV2`` forward at 224, bf16, img/s;
  - one head-training step of ``build_model(224, 224, 3, 5)``: forward, CE,
    backward, Adam.

The stem from uint8 (``stem_u8`` row): ``stem3_u8_fwd_ep`` vs
``normalize_u8_bf16`` + the ``Conv2d`` module + the ``BatchNormAct2d`` eval
forward; and the two end-to-end workloads again from the uint8 batch the data
path delivers (``base_fwd_u8``, ``head_step_u8``), default route vs
``DDLW_STEM_U8=0``. Same alternation, same rule
(``mbconv.stem_u8_fusable`` holds the verdict).

Fine-tuning (``--train``, also part of the default run): every distinct
pointwise shape in its three training directions, our kernel against the path
it replaces —
  - ``fwd+stats``: ``pw_conv_fwd_stats`` + ``bn_finalize`` vs library conv +
    ``bn_stats``;
  - ``dgrad`` / ``wgrad``: ``pw_conv_dgrad`` / ``pw_conv_wgrad`` vs
    ``aten.convolution_backward`` with the matching output mask;
and one training step of ``build_model(224, 224, 3, 5, fine_tune_at=k)`` for
k = 13 and 3, default route vs ``DDLW_PW_TRAIN=0`` (the previous behaviour).
Same protocol, same rule (``binding.pw_train_route`` holds the verdicts).

The training stem from uint8 (``stem_u8_train`` row, ``scratch_step_u8``):
``_StemU8BnActFn`` forward + backward vs ``normalize_u8_input`` + the
``Conv2d`` module + ``BatchNormAct2d`` in training mode, and one from-scratch
step (``fine_tune_at=0``) from a uint8 batch, ``DDLW_STEM_U8_TRAIN=1`` vs
``=0``. Same alternation, same rule (``mbconv.stem_u8_train_enabled`` holds
the verdict); ``--only-stem-u8-train`` runs just these two.

The facade (``facade_head_step_u8``): the head-training step from a uint8
batch through ``train.Model(precision="bf16")`` with the metrics read back
every step (``train_step``) and kept on the device (the ``fit``-path step),
through ``Model(precision="fp32")`` on the normalized fp32 batch, and as the
hand loop — four contenders alternating. The optimizer (``adadelta_step_*``): one
``FusedAdadelta`` step vs ``torch.optim.Adadelta(foreach=True)`` over the fp32
trainable parameters of ``fine_tune_at=13`` and of the head alone; recorded
only.

Run on an MI355X:  python bench/bench_mobilenet.py [--batch 64]
Prints one JSON line per layer shape, a table, and one final JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from ddlw_amd.models.mobilenet_v2 import _V2_CFG, MobileNetV2, build_model  # noqa: E402
from ddlw_amd.ops import (FusedAdadelta, FusedAdam, apply_bf16_policy,  # noqa: E402
                          binding, softmax_cross_entropy)
from ddlw_amd.ops.conv import Conv2d  # noqa: E402
from ddlw_amd.ops.layers import BatchNormAct2d  # noqa: E402

ACTS = ("none", "relu", "relu6")


def layer_shapes(size: int = 224):
    """Distinct pointwise (H, C, K, act, res) and depthwise (H, C, stride)
    layers of MobileNetV2 at ``size`` input, in network order."""
    pw, dw = [], []

    def add(lst, item):
        if item not in lst:
            lst.append(item)

    h, in_ch = size // 2, 32
    for t, c, n, s in _V2_CFG:
        for i in range(n):
            stride = s if i == 0 else 1
            hidden = in_ch * t
            if t != 1:
                add(pw, (h, in_ch, hidden, 2, False))
            add(dw, (h, hidden, stride))
            h = (h + 2 - 3) // stride + 1
            add(pw, (h, hidden, c, 0, stride == 1 and in_ch == c))
            in_ch = c
    add(pw, (h, in_ch, 1280, 2, False))
    return pw, dw


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _round_ms(fn, iters: int) -> float:
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def time_interleaved(fns: dict, iters: int, rounds: int, warmup: int = 3) -> dict:
    """{name: [ms per round]}; the variants alternate round by round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(_round_ms(fn, iters))
    return samples


def _verdict(samples: dict) -> dict:
    fused, unfused = samples["fused"], samples["unfused"]
    mf, mu = statistics.median(fused), statistics.median(unfused)
    spread = max(unfused) - min(unfused)
    return {"ms_fused": round(mf, 4), "ms_unfused": round(mu, 4),
            "ms_min_fused": round(min(fused), 4),
            "spread_unfused": round(spread, 4),
            "speedup": round(mu / mf, 2), "keep": bool(mu - mf > spread)}


def _bn(c, act, dev):
    bn = BatchNormAct2d(c, act=ACTS[act]).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    return bn


def bench_pointwise(B, H, C, K, act, res, dev, iters, rounds):
    torch.manual_seed(0)
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    conv = Conv2d(C, K, 1, bias=False).to(dev).to(torch.bfloat16).eval()
    bn = _bn(K, act, dev)
    r = _cl(torch.randn(B, K, H, H, device=dev).to(torch.bfloat16)) if res else None
    scale, bias = bn.folded_scale_bias()

    def fused():
        return binding.pw_conv_fwd(x, conv.weight, scale, bias, act, r)

    def unfused():
        y = bn(conv(x))
        return r + y if res else y

    with torch.no_grad():
        ref = unfused().float()
        err = ((fused().float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
        rec = _verdict(time_interleaved({"fused": fused, "unfused": unfused},
                                        iters, rounds))
    M = B * H * H
    bytes_io = 2.0 * M * (C + K * (2 if res else 1))
    rec = {"kind": "pointwise", "shape": f"m{M}_c{C}_k{K}", "M": M, "C": C,
           "K": K, "act": act, "res": res, "rel_err_vs_unfused": round(err, 5),
           **rec, "gbps_fused": round(bytes_io / rec["ms_fused"] / 1e6, 1)}
    return rec


def bench_depthwise(B, H, C, stride, dev, iters, rounds):
    torch.manual_seed(0)
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    w = torch.randn(C, 1, 3, 3, device=dev).to(torch.bfloat16)
    bn = _bn(C, 2, dev)
    scale, bias = bn.folded_scale_bias()

    def fused():
        return binding.depthwise_fwd_ep(x, w, scale, bias, 2, stride, 1)

    def unfused():
        return bn(binding.depthwise_fwd(x, w, stride, 1))

    with torch.no_grad():
        ref = unfused().float()
        err = ((fused().float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
        rec = _verdict(time_interleaved({"fused": fused, "unfused": unfused},
                                        iters, rounds))
    Ho = (H + 2 - 3) // stride + 1
    bytes_io = 2.0 * B * C * (H * H + Ho * Ho)
    return {"kind": "depthwise", "shape": f"n{B}_h{H}_c{C}_s{stride}",
            "rel_err_vs_unfused": round(err, 5), **rec,
            "gbps_fused": round(bytes_io / rec["ms_fused"] / 1e6, 1)}


def bench_stem_u8(B, size, dev, iters, rounds):
    """The stem from a uint8 batch: ``stem3_u8_fwd_ep`` ("fused") against the
    path it replaces ("unfused"): ``normalize_u8_bf16``, the 3->32 ``Conv2d``
    module, the ``BatchNormAct2d`` eval forward."""
    from ddlw_amd.ops import mbconv, normalize_u8_bf16

    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, size, size, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    conv = Conv2d(3, 32, 3, stride=2, padding=1, bias=False).to(dev)
    conv = conv.to(torch.bfloat16).to(memory_format=torch.channels_last).eval()
    bn = _bn(32, 2, dev)
    scale, bias = bn.folded_scale_bias()
    wp = mbconv._stem3_packed(conv)

    def fused():
        return binding.stem3_u8_fwd_ep(x, conv.weight, scale, bias, 2, wp=wp)

    def unfused():
        return bn(conv(normalize_u8_bf16(x)))

    with torch.no_grad():
        ref = unfused().float()
        err = ((fused().float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
        rec = _verdict(time_interleaved({"fused": fused, "unfused": unfused},
                                        iters, rounds))
    Ho = (size - 1) // 2 + 1
    bytes_io = 3.0 * B * size * size + 2.0 * B * Ho * Ho * 32
    return {"kind": "stem_u8", "shape": f"n{B}_h{size}_c3_k32_s2",
            "rel_err_vs_unfused": round(err, 5), **rec,
            "gbps_fused": round(bytes_io / rec["ms_fused"] / 1e6, 1)}


def _conv_backward(dy, x, w, mask):
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)


def bench_pointwise_train(B, H, C, K, dev, iters, rounds):
    """fwd+stats, dgrad and wgrad of one pointwise shape: ours ("fused" in the
    verdict's keys) against the library path it replaces ("unfused")."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    dy = _cl(torch.randn(B, K, H, H, device=dev).to(torch.bfloat16))
    w = (torch.randn(K, C, 1, 1, device=dev) / C ** 0.5).to(torch.bfloat16)
    w = w.contiguous(memory_format=torch.channels_last)
    rm = torch.zeros(K, device=dev)
    rv = torch.ones(K, device=dev)
    M = B * H * H
    eps, mom = 1e-5, 0.1

    def fwd_ours():
        y, ps, pq, nparts = binding.pw_conv_fwd_stats(x, w)
        return y, binding.bn_finalize_parts(ps, pq, nparts, M, K, eps, mom, rm, rv)

    def fwd_lib():
        y = F.conv2d(x, w)
        return y, binding.bn_stats(y, eps, mom, rm, rv)

    contenders = {
        "fwd+stats": (fwd_ours, fwd_lib, 2.0 * M * (C + K)),
        "dgrad": (lambda: binding.pw_conv_dgrad(dy, w, x.shape),
                  lambda: _conv_backward(dy, x, w, [True, False, False])[0],
                  2.0 * M * (C + K)),
        "wgrad": (lambda: binding.pw_conv_wgrad(dy, x, w.shape),
                  lambda: _conv_backward(dy, x, w, [False, True, False])[1],
                  2.0 * M * (C + K)),
    }
    recs = []
    with torch.no_grad():
        for direction, (ours, lib, bytes_io) in contenders.items():
            a, b = ours(), lib()
            a, b = (a[0], b[0]) if direction == "fwd+stats" else (a, b)
            err = ((a.float() - b.float()).abs().max()
                   / (b.float().abs().max() + 1e-6)).item()
            rec = _verdict(time_interleaved({"fused": ours, "unfused": lib},
                                            iters, rounds))
            recs.append({"kind": "pw_" + direction, "shape": f"m{M}_c{C}_k{K}",
                         "M": M, "C": C, "K": K, "rel_err_vs_unfused": round(err, 5),
                         **rec,
                         "gbps_fused": round(bytes_io / rec["ms_fused"] / 1e6, 1)})
    return recs


def _with_env(name, value, fn):
    """fn with ``name=value`` in the environment; what was there before is
    put back afterwards."""
    def run():
        before = os.environ.get(name)
        os.environ[name] = value
        try:
            return fn()
        finally:
            if before is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = before
    return run


def _with_fold(value, fn):
    return _with_env("DDLW_EVAL_FOLD", value, fn)


def bench_finetune_step(B, k, dev, iters, rounds):
    """One training step (forward, CE, backward, Adam) of the transfer model
    with ``features[k:]`` trainable: default route ("fused") vs
    ``DDLW_PW_TRAIN=0`` ("unfused"), alternating in one process; a third
    contender, ``DDLW_CONV=hip`` ("forced"), keeps the table's per-layer
    losers on our kernels too."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16))
    labels = torch.randint(0, 5, (B,), device=dev)
    model = apply_bf16_policy(build_model(224, 224, 3, 5, fine_tune_at=k).to(dev)).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    s = time_interleaved({"fused": _with_env("DDLW_PW_TRAIN", "1", step),
                          "unfused": _with_env("DDLW_PW_TRAIN", "0", step),
                          "forced": _with_env("DDLW_CONV", "hip", step)},
                         iters, rounds)
    rec = _verdict(s)
    rec["ms_forced"] = round(statistics.median(s["forced"]), 4)
    rec["spread_forced"] = round(max(s["forced"]) - min(s["forced"]), 4)
    rec["spread_fused"] = round(max(s["fused"]) - min(s["fused"]), 4)
    for name in ("fused", "unfused"):
        rec[f"img_s_{name}"] = round(B / rec[f"ms_{name}"] * 1e3, 1)
    # acceptance: not slower than the contender by more than its spread
    rec["not_slower"] = bool(rec["ms_fused"] - rec["ms_unfused"] <= rec["spread_unfused"])
    return rec


def bench_stem_u8_train(B, size, dev, iters, rounds):
    """The TRAINING stem from a uint8 batch, forward + backward of the stage:
    ``_StemU8BnActFn`` on a marked net ("fused") against the path an unmarked
    net takes ("unfused"): ``normalize_u8_input``, the 3->32 ``Conv2d``
    module, ``BatchNormAct2d`` in training mode."""
    from ddlw_amd.models.mobilenet_v2 import MobileNetV2
    from ddlw_amd.ops import mbconv

    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, size, size, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    net = apply_bf16_policy(MobileNetV2().to(dev)).train()
    net.features = net.features[:3]              # the stage alone
    conv, bn = net.features[0], net.features[1]
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    Ho = (size - 1) // 2 + 1
    gout = _cl(torch.randn(B, 32, Ho, Ho, device=dev).to(torch.bfloat16))
    params = (conv.weight, bn.weight, bn.bias)

    def run(forward):
        for p in params:
            p.grad = None
        y = forward()
        y.backward(gout)
        return y, [p.grad for p in params]

    def fused():
        return run(lambda: mbconv.stem_u8_train_forward(net, x))

    def unfused():
        return run(lambda: bn(conv(mbconv.normalize_u8_input(x, conv.weight))))

    assert _with_env("DDLW_STEM_U8_TRAIN", "1",
                     lambda: mbconv.stem_u8_train_fusable(net, x))()
    (yf, gf), (yu, gu) = fused(), unfused()
    err = ((yf.float() - yu.float()).abs().max() / (yu.float().abs().max() + 1e-6)).item()
    err_dw = ((gf[0].float() - gu[0].float()).norm() / (gu[0].float().norm() + 1e-30)).item()
    s = time_interleaved({"fused": fused, "unfused": unfused}, iters, rounds)
    rec = _verdict(s)
    rec["spread_fused"] = round(max(s["fused"]) - min(s["fused"]), 4)
    # GB/s over the conv's own I/O (the bytes twice, y written, dy read); the
    # BN passes of the stage move more
    bytes_io = 2 * 3.0 * B * size * size + 2 * 2.0 * B * Ho * Ho * 32
    return {"kind": "stem_u8_tr", "shape": f"n{B}_h{size}_c3_k32_s2",
            "rel_err_vs_unfused": round(err, 5), "rel_l2_dw_vs_unfused": round(err_dw, 5),
            **rec, "gbps_fused": round(bytes_io / rec["ms_fused"] / 1e6, 1)}


def bench_scratch_step_u8(B, dev, iters, rounds):
    """One from-scratch training step (``fine_tune_at=0``: every layer
    trains) on a uint8 batch under the bf16 policy: the marked stem on the
    uint8 stem kernels ("fused", ``DDLW_STEM_U8_TRAIN=1``) vs
    ``DDLW_STEM_U8_TRAIN=0`` ("unfused"), alternating in one process."""
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (B,), device=dev)
    model = apply_bf16_policy(build_model(224, 224, 3, 5, fine_tune_at=0).to(dev)).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    s = time_interleaved({"fused": _with_env("DDLW_STEM_U8_TRAIN", "1", step),
                          "unfused": _with_env("DDLW_STEM_U8_TRAIN", "0", step)},
                         iters, rounds)
    rec = _verdict(s)
    rec["spread_fused"] = round(max(s["fused"]) - min(s["fused"]), 4)
    for name in ("fused", "unfused"):
        rec[f"img_s_{name}"] = round(B / rec[f"ms_{name}"] * 1e3, 1)
    # acceptance: not slower than the contender by more than its spread
    rec["not_slower"] = bool(rec["ms_fused"] - rec["ms_unfused"] <= rec["spread_unfused"])
    return rec


def bench_end_to_end(B, dev, iters, rounds):
    torch.manual_seed(0)
    x = _cl(torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16))
    labels = torch.randint(0, 5, (B,), device=dev)
    base = apply_bf16_policy(MobileNetV2().to(dev)).eval()

    def fwd():
        with torch.no_grad():
            return base(x)

    s = time_interleaved({"fused": _with_fold("1", fwd),
                          "unfused": _with_fold("0", fwd)}, iters, rounds)
    out = {"base_fwd": _verdict(s)}
    for k in ("fused", "unfused"):
        out["base_fwd"][f"img_s_{k}"] = round(B / out["base_fwd"][f"ms_{k}"] * 1e3, 1)
    del base

    model = apply_bf16_policy(build_model(224, 224, 3, 5).to(dev)).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    s = time_interleaved({"fused": _with_fold("1", step),
                          "unfused": _with_fold("0", step)}, iters, rounds)
    out["head_step"] = _verdict(s)
    for k in ("fused", "unfused"):
        out["head_step"][f"img_s_{k}"] = round(B / out["head_step"][f"ms_{k}"] * 1e3, 1)
    return out


def bench_end_to_end_u8(B, dev, iters, rounds):
    """The two end-to-end workloads fed the uint8 batch the data path
    delivers: default route (fused stem, "fused") vs ``DDLW_STEM_U8=0``
    (normalize + conv + ``bn_apply``, "unfused"), alternating."""
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (B,), device=dev)
    base = apply_bf16_policy(MobileNetV2().to(dev)).eval()

    def fwd():
        with torch.no_grad():
            return base(x)

    def pair(fn):
        rec = _verdict(time_interleaved(
            {"fused": _with_env("DDLW_STEM_U8", "1", fn),
             "unfused": _with_env("DDLW_STEM_U8", "0", fn)}, iters, rounds))
        for k in ("fused", "unfused"):
            rec[f"img_s_{k}"] = round(B / rec[f"ms_{k}"] * 1e3, 1)
        return rec

    out = {"base_fwd_u8": pair(fwd)}
    del base

    model = apply_bf16_policy(build_model(224, 224, 3, 5).to(dev)).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    out["head_step_u8"] = pair(step)
    return out


def _stats(samples: dict, B=None) -> dict:
    out = {}
    for k, v in samples.items():
        out[f"ms_{k}"] = round(statistics.median(v), 4)
        out[f"spread_{k}"] = round(max(v) - min(v), 4)
        if B is not None:
            out[f"img_s_{k}"] = round(B / statistics.median(v) * 1e3, 1)
    return out


def bench_facade_step(B, dev, iters, rounds):
    """The head-training step of ``build_model(224, 224, 3, 5)`` from a uint8
    batch, four ways, alternating: ``train.Model(precision="bf16")``
    ("facade_bf16", ``train_step``: loss and accuracy read back every step),
    the same model's ``fit``-path step with the metrics on the device
    ("facade_bf16_device"), ``Model(precision="fp32")`` on the normalized
    fp32 NCHW batch ("facade_fp32") and the hand loop of
    ``bench_end_to_end_u8`` ("hand"). The claims: the device-metrics median
    beats the per-step median by more than the per-step spread
    (``device_beats_per_step``), and the bf16 median beats the
    fp32 median by more than the fp32 spread (``bf16_beats_fp32``)."""
    from ddlw_amd.train import Model

    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    x32 = (u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()
    labels = torch.randint(0, 5, (B,), device=dev)

    m16 = Model(build_model(224, 224, 3, 5), dev, precision="bf16")
    m16.compile("Adam", learning_rate=1e-3)
    m32 = Model(build_model(224, 224, 3, 5).to(dev), dev, precision="fp32")
    m32.compile("Adam", learning_rate=1e-3)

    hand = apply_bf16_policy(build_model(224, 224, 3, 5).to(dev)).train()
    opt = FusedAdam([p for p in hand.parameters() if p.requires_grad], lr=1e-3)
    xh = u8.permute(0, 3, 1, 2)

    def hand_step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(hand(xh), labels)
        loss.backward()
        opt.step()
        return loss

    # the step as ``fit`` issues it with the metrics on the device: nothing
    # read back, the host held to RUN_AHEAD steps in front of the device
    m16d = Model(build_model(224, 224, 3, 5), dev, precision="bf16")
    m16d.compile("Adam", learning_rate=1e-3)
    ahead = m16d._run_ahead()

    def device_step():
        m16d.train_step_async(u8, labels)
        ahead.tick()

    s = time_interleaved({"facade_bf16": lambda: m16.train_step(u8, labels),
                          "facade_bf16_device": device_step,
                          "facade_fp32": lambda: m32.train_step(x32, labels),
                          "hand": hand_step}, iters, rounds)
    rec = _stats(s, B)
    rec["bf16_beats_fp32"] = bool(
        rec["ms_facade_fp32"] - rec["ms_facade_bf16"] > rec["spread_facade_fp32"])
    rec["facade_minus_hand_ms"] = round(rec["ms_facade_bf16"] - rec["ms_hand"], 4)
    # the routing rule for metrics_on_device=None: beat the per-step facade
    # by more than that contender's spread
    rec["device_beats_per_step"] = bool(
        rec["ms_facade_bf16"] - rec["ms_facade_bf16_device"] > rec["spread_facade_bf16"])
    rec["device_minus_hand_ms"] = round(rec["ms_facade_bf16_device"] - rec["ms_hand"], 4)
    return rec


def bench_adadelta_step(k, dev, iters, rounds):
    """One optimizer step over the trainable fp32 parameters of
    ``build_model(..., fine_tune_at=k)`` (``None``: the head alone):
    ``FusedAdadelta`` ("fused") vs ``torch.optim.Adadelta(foreach=True)``
    ("unfused"). Recorded only: under bf16 the fused kernel is a matter of
    correctness, so no routing depends on it."""
    torch.manual_seed(0)
    model = build_model(224, 224, 3, 5, fine_tune_at=k).to(dev)
    sets = []
    for _ in range(2):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()
              if p.requires_grad]
        for p in ps:
            p.grad = torch.randn_like(p) * 0.01
        sets.append(ps)
    fused = FusedAdadelta(sets[0], lr=1.0)
    stock = torch.optim.Adadelta(sets[1], lr=1.0, foreach=True)
    rec = _verdict(time_interleaved({"fused": fused.step, "unfused": stock.step},
                                    iters, rounds))
    rec["tensors"] = len(sets[0])
    rec["numel"] = sum(p.numel() for p in sets[0])
    return rec


def _table(recs):
    print(f"{'kind':10s} {'shape':24s} {'fused ms':>9s} {'unfused ms':>10s} "
          f"{'spread':>8s} {'speedup':>8s} {'GB/s':>8s} keep")
    for r in recs:
        print(f"{r['kind']:10s} {r['shape']:24s} {r['ms_fused']:9.4f} "
              f"{r['ms_unfused']:10.4f} {r['spread_unfused']:8.4f} "
              f"{r['speedup']:8.2f} {r['gbps_fused']:8.1f} {r['keep']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--e2e-iters", type=int, default=5)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-frozen", action="store_true",
                    help="skip the frozen-model sections")
    ap.add_argument("--skip-train", action="store_true",
                    help="skip the fine-tuning sections")
    ap.add_argument("--skip-facade", action="store_true",
                    help="skip the Model-facade and Adadelta-step sections")
    ap.add_argument("--only-stem-u8-train", action="store_true",
                    help="run only the training-stem-from-uint8 stage and step")
    ap.add_argument("--fine-tune-at", type=int, nargs="*", default=[13, 3])
    ap.add_argument("--out", type=str, default="bench_out/mobilenet_report.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mobilenet: no GPU (timings are only meaningful on the device)")
    dev = torch.device("cuda:0")
    B = args.batch
    if args.only_stem_u8_train:
        args.skip_layers = args.skip_e2e = args.skip_facade = True
    layers = []
    train_layers = []
    stem_train = []
    if args.only_stem_u8_train or (not args.skip_layers and not args.skip_train):
        # the stage is a fraction of a millisecond: ten times the calls per
        # round, so a round is a ~0.1 s window and not a few milliseconds
        rec = bench_stem_u8_train(B, 224, dev, args.iters * 10, args.rounds)
        stem_train.append(rec)
        print(json.dumps(rec), flush=True)
        _table(stem_train)
    if not args.skip_layers and not args.skip_train:
        seen = []
        for (H, C, K, _act, _res) in layer_shapes(224)[0]:
            if (H, C, K) in seen:
                continue
            seen.append((H, C, K))
            for rec in bench_pointwise_train(B, H, C, K, dev, args.iters, args.rounds):
                train_layers.append(rec)
                print(json.dumps(rec), flush=True)
        _table(train_layers)
    if not args.skip_layers and not args.skip_frozen:
        pw, dw = layer_shapes(224)
        for (H, C, K, act, res) in pw:
            rec = bench_pointwise(B, H, C, K, act, res, dev, args.iters, args.rounds)
            layers.append(rec)
            print(json.dumps(rec), flush=True)
        for (H, C, st) in dw:
            rec = bench_depthwise(B, H, C, st, dev, args.iters, args.rounds)
            layers.append(rec)
            print(json.dumps(rec), flush=True)
        _table(layers)
    stem = []
    if not args.skip_layers and not args.skip_frozen:
        rec = bench_stem_u8(B, 224, dev, args.iters, args.rounds)
        stem.append(rec)
        print(json.dumps(rec), flush=True)
        _table(stem)
    finetune = {}
    if not args.skip_e2e and not args.skip_train:
        for k in args.fine_tune_at:
            r = bench_finetune_step(B, k, dev, args.e2e_iters, args.rounds)
            finetune[f"finetune_step_at_{k}"] = r
            print(json.dumps({f"finetune_step_at_{k}": r}), flush=True)
    if args.only_stem_u8_train or (not args.skip_e2e and not args.skip_train):
        r = bench_scratch_step_u8(B, dev, args.e2e_iters, args.rounds)
        finetune["scratch_step_u8"] = r
        print(json.dumps({"scratch_step_u8": r}), flush=True)
    e2e = ({} if args.skip_e2e or args.skip_frozen
           else bench_end_to_end(B, dev, args.e2e_iters, args.rounds))
    if e2e:
        e2e.update(bench_end_to_end_u8(B, dev, args.e2e_iters, args.rounds))
    facade = {}
    if not args.skip_facade:
        r = bench_facade_step(B, dev, args.e2e_iters, args.rounds)
        facade["facade_head_step_u8"] = r
        print(json.dumps({"facade_head_step_u8": r}), flush=True)
        for k, name in ((13, "adadelta_step_at_13"), (None, "adadelta_step_head")):
            r = bench_adadelta_step(k, dev, args.iters, args.rounds)
            facade[name] = r
            print(json.dumps({name: r}), flush=True)
    for name, r in e2e.items():
        print(f"{name:10s} fused {r['ms_fused']:.3f} ms ({r['img_s_fused']} img/s)  "
              f"unfused {r['ms_unfused']:.3f} ms ({r['img_s_unfused']} img/s)  "
              f"spread {r['spread_unfused']:.3f}  speedup {r['speedup']}")
    report = {"bench": "mobilenet_v2_frozen", "batch": B, "layers": layers,
              "train_layers": train_layers, "stem_u8": stem,
              "stem_u8_train": stem_train, **finetune, **e2e, **facade}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(report, indent=2))
    summary = {"bench": "mobilenet_v2_frozen", "batch": B,
               "layers_kept": sum(r["keep"] for r in layers),
               "layers_total": len(layers),
               "layers_lost": [r["shape"] for r in layers if not r["keep"]]}
    summary["train_layers_kept"] = sum(r["keep"] for r in train_layers)
    summary["train_layers_total"] = len(train_layers)
    summary["train_layers_lost"] = [f"{r['kind']}:{r['shape']}" for r in train_layers
                                    if not r["keep"]]
    if stem:
        summary["stem_u8"] = {k: stem[0][k] for k in ("ms_fused", "ms_unfused",
                                                      "spread_unfused", "speedup", "keep")}
    if stem_train:
        summary["stem_u8_train"] = {k: stem_train[0][k] for k in (
            "ms_fused", "ms_unfused", "spread_unfused", "speedup", "keep")}
    for name, r in {**finetune, **e2e}.items():
        summary[name] = {k: r[k] for k in ("ms_fused", "ms_unfused", "img_s_fused",
                                           "img_s_unfused", "speedup")}
    summary.update(facade)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
