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

The depthwise training stage (``dw_fwd+stats`` / ``dw_bwd`` rows,
``dw_train_step_at_13``, ``dw_train_scratch_step_u8``): every distinct
depthwise shape, ``depthwise_fwd_stats`` + finalize vs ``depthwise_fwd`` +
``bn_stats`` and, at stride 1, ``depthwise_bwd_bn`` vs ``bn_bwd_dx`` + dgrad +
wgrad; then the ``fine_tune_at=13`` step and the from-scratch uint8 step,
``DDLW_DW_TRAIN=1`` vs ``=0``. Same alternation, same rule
(``binding.dw_train_route`` holds the per-shape verdicts);
``--only-dw-train`` runs just these.

The facade (``facade_head_step_u8``): the head-training step from a uint8
batch through ``train.Model(precision="bf16")`` with the metrics read back
every step (``train_step``) and kept on the device (the ``fit``-path step),
through ``Model(precision="fp32")`` on the normalized fp32 batch, and as the
hand loop — four contenders alternating. The optimizer (``adadelta_step_*``): one
``FusedAdadelta`` step vs ``torch.optim.Adadelta(foreach=True)`` over the fp32
trainable parameters of ``fine_tune_at=13`` and of the head alone; recorded
only.

The split-reduction pointwise kernel (``--only-pw-deep``, ``pw_deep*`` rows):
the deep 7x7 layers frozen (plain ``k_pw_conv`` vs ``k_pw_conv_deep`` at
mr = 1 and 2), their training directions against what runs today, and the
frozen forward, the head step and the ``fine_tune_at=13`` step with
``DDLW_PW_DEEP`` unset / ``0`` / ``1``. Same alternation, same rule
(``binding.pw_deep_route`` holds the verdicts and the ``mr`` per shape).

The one-kernel inverted residual (``--only-mbconv-fused``, ``mbconv_fused*``
rows): every distinct stride-1 expanded block through its module forward,
``DDLW_MBCONV_FUSED=1`` vs ``=0`` (the three kernels it replaces; the four
stride-2 blocks under ``DDLW_MBCONV_S2`` and the ``t = 1`` block under
``DDLW_MBCONV_T1`` the same way), then the
frozen forward and the head step from a uint8 batch with the switch unset /
``0`` / ``1``. Same alternation, same rule (``binding.mbconv_fused_route``
holds the verdicts).

The fused tail (``--only-tail-gap``, ``tail_gap*`` rows): the 320 -> 1280 conv
+ BN + ReLU6 + global average pool at batch 16 / 64 / 256, ``DDLW_TAIL_GAP=1``
(``k_pw_conv_gap``, also at 1 / 2 / 4 / 8 images per workgroup) vs ``=0``
(``k_pw_conv`` + ``k_gap_fwd``), then the frozen model forward and the head
step from a uint8 batch with the switch unset / ``0`` / ``1``. Same
alternation, same rule (``binding.pw_gap_route`` holds the verdicts).

The fused head (``--only-head-dense``, ``head_dense*`` rows): dropout + dense
1280 -> 5 at batch 16 / 64 / 256 in training mode, ``DDLW_HEAD_DENSE=1``
(``k_head_dense_fwd`` / ``_bwd``) vs ``=0`` (``k_dropout_fwd`` + ``nn.Linear``):
forward only, and forward + ``softmax_ce_metrics`` + backward without and with
dx; then the head step from a uint8 batch with the switch unset / ``0`` /
``1``. Same alternation, same rule (``binding.head_dense_route``).

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


def bench_depthwise_train(B, H, C, stride, dev, iters, rounds):
    """The depthwise training stage of one shape, ours ("fused") against the
    kernels it replaces ("unfused"): forward ``depthwise_fwd_stats`` +
    finalize vs ``depthwise_fwd`` + ``bn_stats``; at stride 1 the backward
    after the reduce, ``depthwise_bwd_bn`` vs ``bn_bwd_dx`` + dgrad + wgrad."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    w = torch.randn(C, 1, 3, 3, device=dev).to(torch.bfloat16)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    gamma = torch.empty(C, device=dev).uniform_(0.5, 1.5)
    beta = torch.empty(C, device=dev).uniform_(2.0, 4.0)
    eps, mom = 1e-5, 0.1
    y = binding.depthwise_fwd(x, w, stride, 1)
    Ho = y.shape[2]
    M = B * Ho * Ho
    dout = _cl(torch.randn(B, C, Ho, Ho, device=dev).to(torch.bfloat16))
    mean, rstd = binding.bn_stats(y, eps, mom, None, None)
    _, mask = binding.bn_apply(y, None, mean, rstd, gamma, beta, 2)
    dbeta, dgamma = binding.bn_bwd_reduce(dout, mask, y, mean, rstd, True)

    def fwd_ours():
        yy, ps, pq, nparts = binding.depthwise_fwd_stats(x, w, stride, 1)
        return yy, binding.bn_finalize_parts(ps, pq, nparts, M, C, eps, mom, rm, rv)

    def fwd_parts():
        yy = binding.depthwise_fwd(x, w, stride, 1)
        return yy, binding.bn_stats(yy, eps, mom, rm, rv)

    def bwd_ours():
        return binding.depthwise_bwd_bn(dout, mask, y, x, w, mean, rstd, gamma,
                                        dbeta, dgamma, True, True)

    def bwd_parts():
        dz, _ = binding.bn_bwd_dx(dout, mask, y, mean, rstd, gamma, dbeta,
                                  dgamma, True, False)
        return (binding.depthwise_dgrad(dz, w, x.shape, stride, 1),
                binding.depthwise_wgrad(dz, x, w.shape, stride, 1))

    # the bytes the fused kernels must move: x read, y written (+ dout, y, x
    # read and dx written by the backward)
    T_in, T = 2.0 * B * H * H * C, 2.0 * M * C
    contenders = {"fwd+stats": (fwd_ours, fwd_parts, T_in + T)}
    if stride == 1:
        contenders["bwd"] = (bwd_ours, bwd_parts, 2 * T + 2 * T_in)
    recs = []
    with torch.no_grad():
        for direction, (ours, parts, bytes_io) in contenders.items():
            a, b = ours()[0], parts()[0]
            err = ((a.float() - b.float()).abs().max()
                   / (b.float().abs().max() + 1e-6)).item()
            s = time_interleaved({"fused": ours, "unfused": parts}, iters, rounds)
            rec = _verdict(s)
            recs.append({"kind": "dw_" + direction, "shape": f"n{B}_h{H}_c{C}_s{stride}",
                         "M": M, "C": C, "rel_err_vs_unfused": round(err, 5), **rec,
                         "spread_fused": round(max(s["fused"]) - min(s["fused"]), 4),
                         "gbps_fused": round(bytes_io / rec["ms_fused"] / 1e6, 1)})
    return recs


def bench_dw_train_step(B, k, dev, iters, rounds, u8=False):
    """One training step with ``features[k:]`` trainable (``k = 0`` on a uint8
    batch is the from-scratch step): ``DDLW_DW_TRAIN=1`` ("fused") vs ``=0``
    ("unfused"), alternating in one process."""
    torch.manual_seed(0)
    if u8:
        x = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8,
                          device=dev).permute(0, 3, 1, 2)
    else:
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

    s = time_interleaved({"fused": _with_env("DDLW_DW_TRAIN", "1", step),
                          "unfused": _with_env("DDLW_DW_TRAIN", "0", step)},
                         iters, rounds)
    rec = _verdict(s)
    rec["spread_fused"] = round(max(s["fused"]) - min(s["fused"]), 4)
    for name in ("fused", "unfused"):
        rec[f"img_s_{name}"] = round(B / rec[f"ms_{name}"] * 1e3, 1)
    rec["not_slower"] = bool(rec["ms_fused"] - rec["ms_unfused"] <= rec["spread_unfused"])
    return rec


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


# The rows of --only-pw-deep: frozen (batch, H, C, K, act, res) and training
# (direction, C, K of the conv, H, what the row runs on today by
# binding.pw_train_route: "lib" or "plain", batch). pw_deep_route does not
# know the direction, so every GEMM it names is measured in each direction
# MobileNetV2 runs it in.
PW_DEEP_FROZEN = [(64, 7, 576, 160, 0, False), (64, 7, 960, 160, 0, True),
                  (64, 7, 960, 320, 0, False), (16, 7, 576, 160, 0, False),
                  (16, 7, 960, 160, 0, True), (16, 7, 960, 320, 0, False),
                  (64, 14, 576, 96, 0, False)]
PW_DEEP_TRAIN = [("fwd+stats", 960, 160, 7, "lib", 64), ("fwd+stats", 960, 320, 7, "lib", 64),
                 ("fwd+stats", 576, 160, 7, "plain", 64), ("dgrad", 160, 960, 7, "lib", 64),
                 ("dgrad", 320, 1280, 7, "lib", 64),
                 ("fwd+stats", 576, 96, 14, "plain", 64), ("dgrad", 96, 576, 14, "plain", 64),
                 ("fwd+stats", 960, 160, 7, "plain", 16), ("fwd+stats", 960, 320, 7, "plain", 16),
                 ("fwd+stats", 576, 160, 7, "plain", 16), ("dgrad", 160, 960, 7, "plain", 16)]


def _deep_verdict(samples: dict, replaced: str) -> dict:
    """Medians of every contender, the spread (max - min) of the one being
    replaced, and per deep variant whether it beats that one by more than
    that spread."""
    old = samples[replaced]
    m_old = statistics.median(old)
    spread = max(old) - min(old)
    rec = {f"ms_{replaced}": round(m_old, 4), f"spread_{replaced}": round(spread, 4)}
    for name, v in samples.items():
        if name != replaced:
            m = statistics.median(v)
            rec[f"ms_{name}"] = round(m, 4)
            rec[f"speedup_{name}"] = round(m_old / m, 2)
            rec[f"win_{name}"] = bool(m_old - m > spread)
    return rec


def bench_pw_deep_frozen(B, H, C, K, act, res, dev, iters, rounds):
    """One frozen pointwise layer on the plain kernel and on the
    split-reduction kernel at mr = 1 and 2, all through the same binding
    body, alternating."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    w = (torch.randn(K, C, 1, 1, device=dev) / C ** 0.5).to(torch.bfloat16)
    scale, bias = _bn(K, act, dev).folded_scale_bias()
    r = _cl(torch.randn(B, K, H, H, device=dev).to(torch.bfloat16)) if res else None
    fns = {name: (lambda mr=mr: binding._pw_conv_fwd(x, w, scale, bias, act, r, None, mr))
           for name, mr in (("plain", None), ("deep1", 1), ("deep2", 2))}
    with torch.no_grad():
        ref = fns["plain"]().float()
        err = max(((fns[n]().float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
                  for n in ("deep1", "deep2"))
        rec = _deep_verdict(time_interleaved(fns, iters, rounds), "plain")
    M = B * H * H
    return {"kind": "pw_deep", "shape": f"m{M}_c{C}_k{K}" + ("_res" if res else ""),
            "M": M, "C": C, "K": K, "rel_err_vs_plain": round(err, 5), **rec}


def bench_pw_deep_train(direction, C, K, H, today, B, dev, iters, rounds):
    """One training direction of the conv C -> K: what runs today (``today``:
    the library path or the plain kernel) against the split-reduction kernel
    at mr = 1 and 2. The dgrad contenders rebuild w^T per call, as
    ``pw_conv_dgrad`` does."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    dy = _cl(torch.randn(B, K, H, H, device=dev).to(torch.bfloat16))
    w = (torch.randn(K, C, 1, 1, device=dev) / C ** 0.5).to(torch.bfloat16)
    w = w.contiguous(memory_format=torch.channels_last)
    rm, rv = torch.zeros(K, device=dev), torch.ones(K, device=dev)
    M = B * H * H
    eps, mom = 1e-5, 0.1

    def fwd(stats_fn):
        y, ps, pq, nparts = stats_fn()
        return y, binding.bn_finalize_parts(ps, pq, nparts, M, K, eps, mom, rm, rv)

    def fwd_lib():
        y = F.conv2d(x, w)
        return y, binding.bn_stats(y, eps, mom, rm, rv)

    if direction == "fwd+stats":
        fns = {"lib": fwd_lib,
               "plain": lambda: fwd(lambda: binding._pw_conv_fwd_stats(x, w, None, None, "bench"))}
        for mr in (1, 2):
            fns[f"deep{mr}"] = lambda mr=mr: fwd(
                lambda: binding.pw_conv_deep_fwd_stats(x, w, mr=mr))
    else:
        fns = {"lib": lambda: (_conv_backward(dy, x, w, [True, False, False])[0],),
               "plain": lambda: (binding._pw_conv_fwd(
                   dy, binding._pw_w2(w).t().contiguous(), None, None, 0, None, None, None),)}
        for mr in (1, 2):
            fns[f"deep{mr}"] = lambda mr=mr: (binding.pw_conv_deep_fwd(
                dy, binding._pw_w2(w).t().contiguous(), mr=mr),)
    fns = {n: f for n, f in fns.items() if n == today or n.startswith("deep")}
    with torch.no_grad():
        ref = fns[today]()[0].float()
        err = max(((fns[n]()[0].float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
                  for n in ("deep1", "deep2"))
        rec = _deep_verdict(time_interleaved(fns, iters, rounds), today)
    return {"kind": "pw_deep_" + direction, "shape": f"m{M}_c{C}_k{K}", "M": M, "C": C,
            "K": K, "today": today, "rel_err_vs_today": round(err, 5), **rec}


def bench_pw_deep_end_to_end(B, dev, iters, rounds):
    """The frozen forward, the head-training step and the fine_tune_at=13
    step with ``DDLW_PW_DEEP`` unset ("default": the measured predicate), ``0``
    ("off") and ``1`` ("forced"), alternating in one process."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16))
    labels = torch.randint(0, 5, (B,), device=dev)
    os.environ.pop("DDLW_PW_DEEP", None)

    def three(fn):
        s = time_interleaved({"default": fn, "off": _with_env("DDLW_PW_DEEP", "0", fn),
                              "forced": _with_env("DDLW_PW_DEEP", "1", fn)}, iters, rounds)
        return {**_deep_verdict(s, "off"),
                "not_slower": bool(statistics.median(s["default"]) - statistics.median(s["off"])
                                   <= max(s["off"]) - min(s["off"]))}

    base = apply_bf16_policy(MobileNetV2().to(dev)).eval()

    def fwd():
        with torch.no_grad():
            return base(x)

    out = {"pw_deep_base_fwd": three(fwd)}
    del base
    for name, k in (("pw_deep_head_step", None), ("pw_deep_finetune_step_at_13", 13)):
        kw = {} if k is None else {"fine_tune_at": k}
        model = apply_bf16_policy(build_model(224, 224, 3, 5, **kw).to(dev)).train()
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = softmax_cross_entropy(model(x), labels)
            loss.backward()
            opt.step()
            return loss

        out[name] = three(step)
        del model, opt
    return out


# The rows of --only-mbconv-fused: the distinct stride-1 expanded blocks of
# MobileNetV2 @224 as (H, Cin, Cout); Chid = 6 * Cin.
MBCONV_FUSED_BLOCKS = [(56, 24, 24), (28, 32, 32), (14, 64, 64), (14, 64, 96),
                       (14, 96, 96), (7, 160, 160), (7, 160, 320)]
# ... then the four stride-2 blocks and the t = 1 block, each on a kernel and
# a switch of its own, as (input H, Cin, Cout, stride, t, switch)
MBCONV_S2_T1_BLOCKS = [(112, 16, 24, 2, 6, "DDLW_MBCONV_S2"),
                       (56, 24, 32, 2, 6, "DDLW_MBCONV_S2"),
                       (28, 32, 64, 2, 6, "DDLW_MBCONV_S2"),
                       (14, 96, 160, 2, 6, "DDLW_MBCONV_S2"),
                       (112, 32, 16, 1, 1, "DDLW_MBCONV_T1")]


def _frozen_block(cin, cout, dev, stride=1, t=6):
    from ddlw_amd.models.mobilenet_v2 import InvertedResidual

    blk = apply_bf16_policy(InvertedResidual(cin, cout, stride, t).to(dev)).eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, BatchNormAct2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return blk


def bench_mbconv_fused_block(B, H, cin, cout, dev, iters, rounds, stride=1, t=6,
                             switch="DDLW_MBCONV_FUSED"):
    """One frozen block through ``InvertedResidual.forward``: the one-kernel
    path (``switch`` at ``1``, "fused") against the kernels it replaces (at
    ``0``, "three"; two for the ``t = 1`` block), alternating. ``rows``
    counts output pixels."""
    torch.manual_seed(0)
    blk = _frozen_block(cin, cout, dev, stride, t)
    x = _cl(torch.randn(B, cin, H, H, device=dev).to(torch.bfloat16))

    def fwd():
        with torch.no_grad():
            return blk(x)

    fns = {"three": _with_env(switch, "0", fwd), "fused": _with_env(switch, "1", fwd)}
    ref = fns["three"]().float()
    err = ((fns["fused"]().float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
    rec = _deep_verdict(time_interleaved(fns, iters, rounds), "three")
    Ho = (H - 1) // stride + 1
    return {"kind": "mbconv_fused", "shape": f"h{H}_c{cin}_h{t * cin}_k{cout}_s{stride}",
            "rows": B * Ho * Ho, "Cin": cin, "Chid": t * cin, "Cout": cout,
            "rel_err_vs_three": round(err, 5), **rec}


def bench_mbconv_fused_end_to_end(B, dev, iters, rounds):
    """The frozen forward and the head-training step from a uint8 batch with
    ``DDLW_MBCONV_FUSED`` unset ("default": the measured predicate), ``0``
    ("off") and ``1`` ("forced"), alternating in one process; then the same
    two workloads with ``DDLW_MBCONV_S2`` and ``DDLW_MBCONV_T1`` unset
    ("default"), both ``0`` ("off": the five blocks on the kernels they ran
    on before) and both ``1`` ("forced")."""
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (B,), device=dev)
    os.environ.pop("DDLW_MBCONV_FUSED", None)

    def three(fn):
        s = time_interleaved({"default": fn, "off": _with_env("DDLW_MBCONV_FUSED", "0", fn),
                              "forced": _with_env("DDLW_MBCONV_FUSED", "1", fn)}, iters, rounds)
        return _deep_verdict(s, "off")

    def both(value, fn):
        return _with_env("DDLW_MBCONV_S2", value, _with_env("DDLW_MBCONV_T1", value, fn))

    def three_new(fn):
        s = time_interleaved({"default": fn, "off": both("0", fn), "forced": both("1", fn)},
                             iters, rounds)
        return _deep_verdict(s, "off")

    base = apply_bf16_policy(MobileNetV2().to(dev)).eval()

    def fwd():
        with torch.no_grad():
            return base(x)

    out = {"mbconv_fused_base_fwd_u8": three(fwd),
           "mbconv_s2_t1_base_fwd_u8": three_new(fwd)}
    del base
    model = apply_bf16_policy(build_model(224, 224, 3, 5).to(dev)).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    out["mbconv_fused_head_step_u8"] = three(step)
    out["mbconv_s2_t1_head_step_u8"] = three_new(step)
    return out


# The rows of --only-tail-gap: the 320 -> 1280 tail + global average pool of
# MobileNetV2 @224 (7x7) at these batches.
TAIL_GAP_BATCHES = [16, 64, 256]


def bench_tail_gap_layer(B, dev, iters, rounds, H=7, C=320, K=1280):
    """The frozen tail conv + BN + ReLU6 + GAP through
    ``mbconv.conv_bn_gap_eval``: ``DDLW_TAIL_GAP=0`` ("pair": ``k_pw_conv`` +
    ``k_gap_fwd``) against ``=1`` ("fused": ``k_pw_conv_gap`` with the host's
    images-per-workgroup choice), and the kernel at imgs = 1, 2, 4, 8,
    alternating."""
    from ddlw_amd.ops import mbconv

    torch.manual_seed(0)
    conv = Conv2d(C, K, 1, bias=False).to(dev).to(torch.bfloat16).eval()
    bn = _bn(K, 2, dev)
    scale, bias = bn.folded_scale_bias()
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))

    def run():
        with torch.no_grad():
            return mbconv.conv_bn_gap_eval(conv, bn, x)

    fns = {"pair": _with_env("DDLW_TAIL_GAP", "0", run),
           "fused": _with_env("DDLW_TAIL_GAP", "1", run)}
    for imgs in (1, 2, 4, 8):
        fns[f"imgs{imgs}"] = (lambda imgs=imgs: binding.pw_conv_gap_fwd(
            x, conv.weight, scale, bias, 2, imgs=imgs))
    ref = fns["pair"]()
    equal = all(torch.equal(fn(), ref) for name, fn in fns.items() if name != "pair")
    rec = _deep_verdict(time_interleaved(fns, iters, rounds), "pair")
    return {"kind": "tail_gap", "shape": f"n{B}_hw{H * H}_c{C}_k{K}", "N": B,
            "imgs_host": binding._pw_gap_imgs(B, K, x.device), "bit_equal": equal, **rec}


def bench_tail_gap_end_to_end(B, dev, iters, rounds):
    """The frozen forward (``build_model`` in eval mode: base, pool, head) and
    the head-training step from a uint8 batch with ``DDLW_TAIL_GAP`` unset
    ("default": the measured table), ``0`` ("off") and ``1`` ("forced"),
    alternating in one process."""
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (B,), device=dev)
    os.environ.pop("DDLW_TAIL_GAP", None)

    def three(fn):
        s = time_interleaved({"default": fn, "off": _with_env("DDLW_TAIL_GAP", "0", fn),
                              "forced": _with_env("DDLW_TAIL_GAP", "1", fn)}, iters, rounds)
        return _deep_verdict(s, "off")

    model = apply_bf16_policy(build_model(224, 224, 3, 5).to(dev)).eval()

    def fwd():
        with torch.no_grad():
            return model(x)

    out = {"tail_gap_model_fwd_u8": three(fwd)}
    model.train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    out["tail_gap_head_step_u8"] = three(step)
    return out


# The rows of --only-head-dense: dropout + dense 1280 -> 5 of the transfer
# head at these batches.
HEAD_DENSE_BATCHES = [16, 64, 256]


def bench_head_dense_stage(B, dev, iters, rounds, C=1280, K=5, p=0.5):
    """The head stage as ``TransferModel.forward`` runs it, in training mode:
    ``DDLW_HEAD_DENSE=0`` ("off": ``k_dropout_fwd`` + ``nn.Linear``) against
    ``=1`` ("fused": ``k_head_dense_fwd`` / ``_bwd``), alternating. Three rows:
    forward only; forward + ``softmax_ce_metrics`` + backward without dx (a
    frozen base) and with dx (a trainable suffix)."""
    from ddlw_amd.ops.layers import (Dropout, dropout_linear, dropout_linear_route,
                                     softmax_ce_metrics)

    torch.manual_seed(0)
    drop = Dropout(p).train()
    lin = torch.nn.Linear(C, K).to(dev).to(torch.bfloat16)
    x = torch.randn(B, C, device=dev).to(torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    labels = torch.randint(0, K, (B,), device=dev)

    def head(xx):
        if dropout_linear_route(xx, drop, lin):
            return dropout_linear(xx, drop, lin)
        return lin(drop(xx))

    def fwd():
        with torch.no_grad():
            return head(x)

    def fwd_bwd(xx):
        def run():
            lin.zero_grad(set_to_none=True)
            xx.grad = None
            loss, _ = softmax_ce_metrics(head(xx), labels)
            loss.backward()
            return loss
        return run

    recs = []
    for what, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd(x)), ("fwd_bwd_dx", fwd_bwd(xg))):
        fns = {"off": _with_env("DDLW_HEAD_DENSE", "0", fn),
               "fused": _with_env("DDLW_HEAD_DENSE", "1", fn)}
        rec = _deep_verdict(time_interleaved(fns, iters, rounds), "off")
        recs.append({"kind": "head_dense", "what": what,
                     "shape": f"n{B}_c{C}_k{K}", "N": B, **rec})
    return recs


def bench_head_dense_end_to_end(B, dev, iters, rounds):
    """The head-training step of ``build_model(224, 224, 3, 5)`` from a uint8
    batch with ``DDLW_HEAD_DENSE`` unset ("default": the measured table), ``0``
    ("off") and ``1`` ("forced"), alternating in one process."""
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    x = u8.permute(0, 3, 1, 2)
    labels = torch.randint(0, 5, (B,), device=dev)
    os.environ.pop("DDLW_HEAD_DENSE", None)
    model = apply_bf16_policy(build_model(224, 224, 3, 5).to(dev)).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        opt.step()
        return loss

    s = time_interleaved({"default": step, "off": _with_env("DDLW_HEAD_DENSE", "0", step),
                          "forced": _with_env("DDLW_HEAD_DENSE", "1", step)}, iters, rounds)
    return {"head_dense_head_step_u8": _deep_verdict(s, "off")}


# The rows of --only-frozen-bn: the distinct stages of features[13:] @224 as
# pointwise (H, C, K, act) and depthwise (H, C, stride).
FROZEN_BN_PW = [(14, 96, 576, 2), (14, 576, 96, 0), (7, 576, 160, 0), (7, 160, 960, 2),
                (7, 960, 160, 0), (7, 960, 320, 0), (7, 320, 1280, 2)]
FROZEN_BN_DW = [(14, 576, 1), (14, 576, 2), (7, 960, 1)]


def bench_frozen_bn_stage(B, H, C, K, act, stride, dev, iters, rounds):
    """The backward of one conv + frozen-BN stage, per direction: the module
    path it replaces ("module": ``_BnActFn`` in eval mode, then the conv
    Function's backward) against the stage Function on the gated kernels
    ("gated", ``DDLW_FROZEN_BN=1``), alternating. Each contender is
    ``autograd.grad`` over a graph built once, with only the timed
    direction's input wanting a gradient (a depthwise stage: both)."""
    from ddlw_amd.ops import mbconv

    torch.manual_seed(0)
    dw = stride > 0
    conv = (Conv2d(C, C, 3, stride=stride, padding=1, groups=C, bias=False) if dw
            else Conv2d(C, K, 1, bias=False)).to(dev).to(torch.bfloat16).eval()
    conv.pw_train = not dw
    bn = _bn(K, act, dev)
    for p in bn.parameters():
        p.requires_grad = False
    x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
    recs = []
    for what in (("bwd",) if dw else ("dgrad", "wgrad")):
        x.requires_grad_(what != "wgrad")
        conv.weight.requires_grad_(what != "dgrad")
        wanted = [t for t in (x, conv.weight) if t.requires_grad]
        y_mod = bn(conv(x))
        y_new = mbconv.conv_bn_frozen(conv, bn, x)
        dout = _cl(torch.randn_like(y_mod) / y_mod.numel() * K)
        fns = {"module": lambda: torch.autograd.grad(y_mod, wanted, dout, retain_graph=True),
               "gated": _with_env("DDLW_FROZEN_BN", "1", lambda: torch.autograd.grad(
                   y_new, wanted, dout, retain_graph=True))}
        rec = _deep_verdict(time_interleaved(fns, iters, rounds), "module")
        M = B * y_mod.shape[2] * y_mod.shape[3]
        kind = "dw_bwd" if dw else "pw_" + what
        recs.append({"kind": "frozen_bn", "what": kind, "C": C, "K": K,
                     "stride": max(stride, 1), "M": M,
                     "shape": f"{H}x{H}_c{C}_k{K}_s{max(stride, 1)}", **rec})
    return recs


def bench_frozen_bn_step(B, dev, iters, rounds, k=13):
    """The ``fine_tune_at=k`` training step under bf16 with
    ``fine_tune_bn="frozen"`` and ``DDLW_FROZEN_BN`` unset ("default": the
    measured table), ``1`` ("forced") and ``0`` ("off": the module path), and,
    for orientation, the ``fine_tune_bn="batch"`` step, alternating in one
    process."""
    torch.manual_seed(0)
    x = _cl(torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16))
    labels = torch.randint(0, 5, (B,), device=dev)
    os.environ.pop("DDLW_FROZEN_BN", None)

    def make(bn_mode):
        model = apply_bf16_policy(build_model(
            224, 224, 3, 5, fine_tune_at=k, fine_tune_bn=bn_mode).to(dev)).train()
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = softmax_cross_entropy(model(x), labels)
            loss.backward()
            opt.step()
            return loss
        return step

    frozen, batch = make("frozen"), make("batch")
    s = time_interleaved({"default": frozen, "off": _with_env("DDLW_FROZEN_BN", "0", frozen),
                          "forced": _with_env("DDLW_FROZEN_BN", "1", frozen),
                          "batch": batch}, iters, rounds)
    return {f"frozen_bn_step_at_{k}": _deep_verdict(s, "off")}


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
    ap.add_argument("--only-dw-train", action="store_true",
                    help="run only the depthwise training stage rows and steps")
    ap.add_argument("--only-pw-deep", action="store_true",
                    help="run only the split-reduction pointwise rows and steps")
    ap.add_argument("--only-mbconv-fused", action="store_true",
                    help="run only the one-kernel inverted residual rows and steps")
    ap.add_argument("--only-tail-gap", action="store_true",
                    help="run only the fused tail conv + GAP rows and steps")
    ap.add_argument("--only-head-dense", action="store_true",
                    help="run only the fused dropout + dense head rows and step")
    ap.add_argument("--only-frozen-bn", action="store_true",
                    help="run only the frozen-BN backward rows and fine-tuning steps")
    ap.add_argument("--fine-tune-at", type=int, nargs="*", default=[13, 3])
    ap.add_argument("--out", type=str, default="bench_out/mobilenet_report.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mobilenet: no GPU (timings are only meaningful on the device)")
    dev = torch.device("cuda:0")
    B = args.batch
    if (args.only_stem_u8_train or args.only_dw_train or args.only_pw_deep
            or args.only_mbconv_fused or args.only_tail_gap or args.only_head_dense
            or args.only_frozen_bn):
        args.skip_layers = args.skip_e2e = args.skip_facade = True
    pw_deep = {}
    if args.only_frozen_bn:
        rows = [rec for (H, C, K, act) in FROZEN_BN_PW
                for rec in bench_frozen_bn_stage(B, H, C, K, act, 0, dev, args.iters, args.rounds)]
        rows += [rec for (H, C, st) in FROZEN_BN_DW
                 for rec in bench_frozen_bn_stage(B, H, C, C, 2, st, dev, args.iters, args.rounds)]
        for rec in rows:
            print(json.dumps(rec), flush=True)
        pw_deep = {"frozen_bn_stages": rows,
                   **bench_frozen_bn_step(B, dev, args.e2e_iters, args.rounds)}
        print(json.dumps({k: v for k, v in pw_deep.items() if k != "frozen_bn_stages"}),
              flush=True)
    if args.only_head_dense:
        # the stage is tens of microseconds: ten times the calls per round
        rows = [rec for b in HEAD_DENSE_BATCHES
                for rec in bench_head_dense_stage(b, dev, args.iters * 10, args.rounds)]
        for rec in rows:
            print(json.dumps(rec), flush=True)
        pw_deep = {"head_dense_stage": rows,
                   **bench_head_dense_end_to_end(B, dev, args.e2e_iters, args.rounds)}
        print(json.dumps({k: v for k, v in pw_deep.items() if k != "head_dense_stage"}),
              flush=True)
    if args.only_tail_gap:
        # the pair is tens of microseconds: ten times the calls per round
        rows = [bench_tail_gap_layer(b, dev, args.iters * 10, args.rounds)
                for b in TAIL_GAP_BATCHES]
        for rec in rows:
            print(json.dumps(rec), flush=True)
        pw_deep = {"tail_gap_layers": rows,
                   **bench_tail_gap_end_to_end(B, dev, args.e2e_iters, args.rounds)}
        for name, r in pw_deep.items():
            if name != "tail_gap_layers":
                print(json.dumps({name: r}), flush=True)
    if args.only_mbconv_fused:
        rows = [bench_mbconv_fused_block(B, *row, dev, args.iters, args.rounds)
                for row in MBCONV_FUSED_BLOCKS]
        rows += [bench_mbconv_fused_block(B, H, cin, cout, dev, args.iters, args.rounds,
                                          stride, t, switch)
                 for H, cin, cout, stride, t, switch in MBCONV_S2_T1_BLOCKS]
        for rec in rows:
            print(json.dumps(rec), flush=True)
        pw_deep = {"mbconv_fused_blocks": rows,
                   **bench_mbconv_fused_end_to_end(B, dev, args.e2e_iters, args.rounds)}
        for name, r in pw_deep.items():
            if name != "mbconv_fused_blocks":
                print(json.dumps({name: r}), flush=True)
    if args.only_pw_deep:
        rows = [bench_pw_deep_frozen(*row, dev, args.iters, args.rounds)
                for row in PW_DEEP_FROZEN]
        rows += [bench_pw_deep_train(*row, dev, args.iters, args.rounds)
                 for row in PW_DEEP_TRAIN]
        for rec in rows:
            print(json.dumps(rec), flush=True)
        pw_deep = {"pw_deep_layers": rows,
                   **bench_pw_deep_end_to_end(B, dev, args.e2e_iters, args.rounds)}
        for name, r in pw_deep.items():
            if name != "pw_deep_layers":
                print(json.dumps({name: r}), flush=True)
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
    dw_train = []
    if args.only_dw_train or (not args.skip_layers and not args.skip_train):
        for (H, C, st) in layer_shapes(224)[1]:
            for rec in bench_depthwise_train(B, H, C, st, dev, args.iters, args.rounds):
                dw_train.append(rec)
                print(json.dumps(rec), flush=True)
        _table(dw_train)
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
    if args.only_dw_train or (not args.skip_e2e and not args.skip_train):
        for name, k, u8 in (("dw_train_step_at_13", 13, False),
                            ("dw_train_scratch_step_u8", 0, True)):
            r = bench_dw_train_step(B, k, dev, args.e2e_iters, args.rounds, u8=u8)
            finetune[name] = r
            print(json.dumps({name: r}), flush=True)
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
              "train_layers": train_layers, "dw_train_layers": dw_train,
              "stem_u8": stem,
              "stem_u8_train": stem_train, **finetune, **e2e, **facade, **pw_deep}
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
    summary.update({k: v for k, v in pw_deep.items()
                    if k not in ("pw_deep_layers", "mbconv_fused_blocks",
                                 "tail_gap_layers", "frozen_bn_stages")})
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
