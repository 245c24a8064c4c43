"""Eval-mode MobileNetV2 inverted residual on fused kernels — the MobileNetV2
counterpart of ``bottleneck_eval_forward`` in ``ops/block.py``.

In a frozen base every BN is a constant per-channel affine, so it rides the
epilogue of the conv before it: an expanded block is three kernels
(pointwise MFMA expand + ReLU6, depthwise + ReLU6, pointwise project +
residual) instead of conv / bn_apply pairs and an eager add. Fed a uint8
batch, the frozen stem (normalize, 3->32 conv, BN, ReLU6) is one kernel too.

A training-mode block (the fine-tuned suffix) runs its two pointwise stages on
``_PwConvBnActFn``: the conv kernel emits the BN statistics from its epilogue
and the backward runs on the pointwise dgrad and the split-K wgrad kernels.
A marked training stem fed a uint8 batch runs on ``_StemU8BnActFn`` the same
way, its forward and its weight gradient reading the bytes.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import binding

_ACT = {"none": 0, "relu": 1, "relu6": 2}


def eval_fold_enabled(module, x: torch.Tensor) -> bool:
    """The conditions under which a frozen module may take the folded-BN
    kernels: eval mode, no grad, CUDA bf16 input, and none of the three
    environment switches set (all read at call time)."""
    if module.training or torch.is_grad_enabled():
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return False
    if os.environ.get("DDLW_DISABLE_HIP_OPS", "0") == "1":
        return False
    if os.environ.get("DDLW_EVAL_FOLD", "1") != "1":
        return False
    if os.environ.get("DDLW_CONV", "auto") == "stock":
        return False
    return True


def _bn_fp32(bn) -> bool:
    return (bn.running_mean.dtype == torch.float32
            and bn.running_var.dtype == torch.float32)


def _stages(block):
    """[(conv, bn)] of a block's ``conv`` Sequential, in order."""
    mods = [m for m in block.conv if not isinstance(m, torch.nn.Identity)]
    return list(zip(mods[0::2], mods[1::2]))


def inverted_residual_eval_fusable(block, x: torch.Tensor) -> bool:
    if not eval_fold_enabled(block, x):
        return False
    return all(_bn_fp32(bn) for _, bn in _stages(block))


def _is_pointwise(conv) -> bool:
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1
            and conv.bias is None)


def _is_depthwise3x3(conv) -> bool:
    return (conv.groups == conv.in_channels == conv.out_channels
            and conv.kernel_size == (3, 3) and conv.stride in ((1, 1), (2, 2))
            and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.bias is None and conv.in_channels % 8 == 0)


def conv_bn_eval(conv, bn, x: torch.Tensor, res=None) -> torch.Tensor:
    """One conv + BatchNormAct2d stage of a frozen block: on the fused
    kernel when its shape is supported, else unfused
    (the module path: conv, then ``bn_apply``), for that stage only."""
    act = _ACT[bn.act]
    if _is_pointwise(conv):
        if binding.pw_conv_supported(conv.in_channels, conv.out_channels):
            scale, bias = bn.folded_scale_bias()
            return binding.pw_conv_fwd(x, conv.weight, scale, bias, act, res)
    elif _is_depthwise3x3(conv) and res is None:
        scale, bias = bn.folded_scale_bias()
        return binding.depthwise_fwd_ep(x, conv.weight, scale, bias, act,
                                        conv.stride[0], conv.padding[0])
    y = bn(conv(x))
    return y if res is None else res + y


@torch.no_grad()
def inverted_residual_eval_forward(block, x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous(memory_format=torch.channels_last)
    stages = _stages(block)
    h = x
    for conv, bn in stages[:-1]:
        h = conv_bn_eval(conv, bn, h)
    conv, bn = stages[-1]
    return conv_bn_eval(conv, bn, h, res=x if block.use_res else None)


# --------------------------------------------------------------------------- #
# Stem from a uint8 image batch: normalize + conv + BN + ReLU6 in one kernel
# --------------------------------------------------------------------------- #


def _is_stem3(conv) -> bool:
    return (conv.in_channels == 3 and conv.out_channels == 32
            and conv.kernel_size == (3, 3) and conv.stride == (2, 2)
            and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None
            and conv.weight.dtype == torch.bfloat16)


def stem_u8_fusable(net, x) -> bool:
    """The conditions under which ``net.features[0:3]`` (stem conv,
    BatchNormAct2d, the old ReLU6 slot) of a MobileNetV2 takes a uint8 batch
    on ``binding.stem3_u8_fwd_ep``: ``eval_fold_enabled``'s with uint8 in
    place of bf16 (stem children in eval mode, no grad, CUDA input, the three
    switches), fp32 BN statistics, the 3->32 3x3 stride-2 pad-1 bias-free
    conv with bf16 weights, a channels_last batch, and the A/B switch
    ``DDLW_STEM_U8`` (default ``1``) not ``0``. All read at call time.
    No measured-loser predicate: the fused stem beat normalize + conv +
    ``bn_apply`` by more than their spread at batch 64 / 224
    (bench/bench_mobilenet.py; rows in docs/KERNELS.md)."""
    if torch.is_grad_enabled() or any(m.training for m in net.features[:3]):
        return False
    if not (x.is_cuda and x.dtype == torch.uint8):
        return False
    if os.environ.get("DDLW_DISABLE_HIP_OPS", "0") == "1":
        return False
    if os.environ.get("DDLW_EVAL_FOLD", "1") != "1":
        return False
    if os.environ.get("DDLW_CONV", "auto") == "stock":
        return False
    if os.environ.get("DDLW_STEM_U8", "1") == "0":
        return False
    conv, bn = net.features[0], net.features[1]
    if not (_is_stem3(conv) and _bn_fp32(bn)):
        return False
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


def _stem_trains(conv, bn) -> bool:
    """A stem with a parameter that wants a gradient: its weight, BN affine
    and running statistics move under the kernels (fused optimizers,
    ``bn_finalize``), which write through raw pointers and bump no
    ``_version``, so nothing derived from them may be cached."""
    return (conv.weight.requires_grad or bn.weight.requires_grad
            or bn.bias.requires_grad)


def _stem3_packed(conv, fresh: bool = False) -> torch.Tensor:
    """``binding.stem3_pack_weight(conv.weight)``, cached on the module until
    the weight mutates or moves (as ``folded_scale_bias`` caches);
    ``fresh=True`` packs the live weight and leaves the cache alone."""
    w = conv.weight
    if fresh:
        return binding.stem3_pack_weight(w)
    key = (w._version, w.data_ptr(), w.device)
    cached = getattr(conv, "_stem3_cache", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    wp = binding.stem3_pack_weight(w)
    conv._stem3_cache = (key, wp)
    return wp


@torch.no_grad()
def stem_u8_forward(net, x: torch.Tensor, fresh: bool = False) -> torch.Tensor:
    """``features[0:3]`` of a MobileNetV2 in eval mode on a uint8 batch: one
    launch (``stem_u8_fusable`` is the caller's to check). A frozen stem
    uses the cached weight pack and BN fold. ``fresh=True`` is for a
    trainable stem that is being evaluated between training steps
    (validation during ``fit``): its weight, BN affine and running statistics
    move under kernels that bump no ``_version``, so the pack and the fold
    are computed from the live tensors on every call."""
    conv, bn = net.features[0], net.features[1]
    scale, bias = bn.folded_scale_bias(fresh=fresh)
    return binding.stem3_u8_fwd_ep(x, conv.weight, scale, bias, _ACT[bn.act],
                                   wp=_stem3_packed(conv, fresh=fresh))


# Measured loser by the project's rule (docs/KERNELS.md, "MobileNetV2 stem from
# uint8, training"): at batch 64 / 224 the stage ran 1.03-1.10x the module
# path's speed on medians in three runs, by more than that path's spread in
# only one of them, and the from-scratch step stayed inside its spread. So
# the route is opt-in twice: the mark, and this switch.
_STEM_U8_TRAIN_DEFAULT = "0"


def stem_u8_train_enabled() -> bool:
    """The A/B switch of the training-mode uint8 stem, read at call time:
    ``DDLW_STEM_U8_TRAIN=1`` puts a marked training stem on the stage
    Function, ``0`` (the default, see above) leaves it on normalize + module
    conv + BatchNormAct2d."""
    return os.environ.get("DDLW_STEM_U8_TRAIN", _STEM_U8_TRAIN_DEFAULT) != "0"


def stem_u8_train_fusable(net, x) -> bool:
    """The conditions under which a TRAINING stem (``net.features[0:3]``)
    takes a uint8 batch on ``_StemU8BnActFn``: the opt-in mark on the stem
    conv (``Conv2d.u8_train``, set by ``MobileNetV2.enable_u8_train_stem``,
    which ``apply_bf16_policy`` calls), grad enabled, the stem BN in training
    mode, a gradient wanted by the conv weight or the BN affine, a CUDA uint8
    channels_last 4-D batch, the 3->32 3x3 stride-2 pad-1 bias-free conv with
    bf16 weights, fp32 BN statistics, neither of ``DDLW_DISABLE_HIP_OPS=1``
    and ``DDLW_CONV=stock``, and ``DDLW_STEM_U8_TRAIN=1`` (default ``0``,
    ``stem_u8_train_enabled``). All read at call time."""
    conv, bn = net.features[0], net.features[1]
    if not getattr(conv, "u8_train", False):
        return False
    if not (torch.is_grad_enabled() and bn.training):
        return False
    if not _stem_trains(conv, bn):
        return False
    if not (x.is_cuda and x.dtype == torch.uint8):
        return False
    if os.environ.get("DDLW_DISABLE_HIP_OPS", "0") == "1":
        return False
    if os.environ.get("DDLW_CONV", "auto") == "stock":
        return False
    if not stem_u8_train_enabled():
        return False
    if not (_is_stem3(conv) and _bn_fp32(bn)):
        return False
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


class _StemU8BnActFn(torch.autograd.Function):
    """normalize -> conv3x3/s2 -> BatchNormAct2d of a training-mode stem fed
    a uint8 batch; mirrors ``_PwConvBnActFn``. Forward: the stem kernel reads
    the bytes and writes the conv output and its BN statistics partials in
    one pass (no normalized batch, no ``k_bn_stats`` re-read), ``bn_finalize``
    turns them into mean / rstd and updates the running buffers, ``bn_apply``
    normalizes. Backward: BN reduce, BN dx, then the weight gradient from the
    bytes again. No dx: the stem is the first layer."""

    @staticmethod
    def forward(ctx, x_u8, weight, wp, gamma, beta, running_mean, running_var,
                momentum: float, eps: float, act: int):
        k = weight.shape[0]
        y, ps, pq, nparts = binding.stem3_u8_fwd_stats(x_u8, weight, wp=wp)
        rows = y.shape[0] * y.shape[2] * y.shape[3]
        mean, rstd = binding.bn_finalize_parts(
            ps, pq, nparts, rows, k, eps, momentum, running_mean, running_var)
        out, mask = binding.bn_apply(y, None, mean, rstd, gamma, beta, act)
        if mask is None:
            mask = x_u8.new_empty(0, dtype=torch.uint8)
        ctx.save_for_backward(x_u8, y, mask, mean, rstd, gamma)
        ctx.relu = bool(act)  # the mask bit means "gradient passes"
        ctx.weight_shape = tuple(weight.shape)
        ctx.weight_dtype = weight.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        x_u8, y, mask, mean, rstd, gamma = ctx.saved_tensors
        dout = dout.contiguous(memory_format=torch.channels_last)
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        dbeta, dgamma = binding.bn_bwd_reduce(dout, mask, y, mean, rstd, ctx.relu)
        dw = None
        if ctx.needs_input_grad[1]:
            dy, _ = binding.bn_bwd_dx(dout, mask, y, mean, rstd, gamma, dbeta,
                                      dgamma, ctx.relu, False)
            dw = binding.stem3_u8_wgrad(x_u8, dy, ctx.weight_shape).to(ctx.weight_dtype)
        return None, dw, None, dgamma, dbeta, None, None, None, None, None


def stem_u8_train_forward(net, x: torch.Tensor) -> torch.Tensor:
    """``features[0:3]`` of a training MobileNetV2 on a uint8 batch, on the
    stage Function (``stem_u8_train_fusable`` is the caller's to check); the
    BN module's bookkeeping is done here as its forward does. The weight is
    packed anew on every call (864 values): the optimizer kernels update it
    without a ``_version`` bump, so a cached pack would be the first step's."""
    conv, bn = net.features[0], net.features[1]
    bn.num_batches_tracked += 1
    w, b = bn.weight, bn.bias
    if w.dtype != torch.float32:
        w, b = w.float(), b.float()
    return _StemU8BnActFn.apply(x, conv.weight, _stem3_packed(conv, fresh=True), w, b,
                                bn.running_mean, bn.running_var, bn.momentum,
                                bn.eps, _ACT[bn.act])


def normalize_u8_input(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The ``preprocess_input`` normalize of a uint8 batch for a stem the
    fused kernel does not take: ``normalize_u8_bf16`` (what callers ran
    themselves) for bf16 stem weights on CUDA, else fp32 ``x / 127.5 - 1``
    (``data.preprocess.normalize_uint8``) cast to the weight's dtype."""
    if x.is_cuda and weight.dtype == torch.bfloat16:
        from .layers import normalize_u8_bf16

        if x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        return normalize_u8_bf16(x)
    return (x.to(torch.float32) / 127.5 - 1.0).to(weight.dtype)


# --------------------------------------------------------------------------- #
# Training-mode block: pointwise conv + BatchNorm stages on one Function
# --------------------------------------------------------------------------- #


class _PwConvBnActFn(torch.autograd.Function):
    """conv1x1 -> BatchNormAct2d of a training-mode block. Forward: the
    pointwise kernel writes the conv output and its BN statistics partials
    in one pass (no ``k_bn_stats`` re-read), ``bn_finalize`` turns them into
    mean / rstd and updates the running buffers, ``bn_apply`` normalizes.
    Backward: BN reduce, BN dx, then the conv's dgrad and wgrad."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var,
                momentum: float, eps: float, act: int):
        x = x.contiguous(memory_format=torch.channels_last)
        k, c = weight.shape[0], weight.shape[1]
        rows = x.shape[0] * x.shape[2] * x.shape[3]
        if binding.pw_train_route("fwd", c, k, rows):
            y, ps, pq, nparts = binding.pw_conv_fwd_stats(x, weight)
            mean, rstd = binding.bn_finalize_parts(
                ps, pq, nparts, rows, k, eps, momentum, running_mean,
                running_var)
        else:
            y = F.conv2d(x, weight.to(x.dtype))
            y = y.contiguous(memory_format=torch.channels_last)
            mean, rstd = binding.bn_stats(y, eps, momentum, running_mean,
                                          running_var)
        out, mask = binding.bn_apply(y, None, mean, rstd, gamma, beta, act)
        if mask is None:
            mask = x.new_empty(0, dtype=torch.uint8)
        ctx.save_for_backward(x, weight, y, mask, mean, rstd, gamma)
        ctx.relu = bool(act)  # the mask bit means "gradient passes"
        return out

    @staticmethod
    def backward(ctx, dout):
        from .conv import pw_conv_backward

        x, weight, y, mask, mean, rstd, gamma = ctx.saved_tensors
        dout = dout.contiguous(memory_format=torch.channels_last)
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        dbeta, dgamma = binding.bn_bwd_reduce(dout, mask, y, mean, rstd, ctx.relu)
        dy, _ = binding.bn_bwd_dx(dout, mask, y, mean, rstd, gamma, dbeta,
                                  dgamma, ctx.relu, False)
        dx, dw = pw_conv_backward(dy, x, weight, ctx.needs_input_grad[0],
                                  ctx.needs_input_grad[1])
        return dx, dw, dgamma, dbeta, None, None, None, None, None


def pw_conv_bn_train(conv, bn, x: torch.Tensor) -> torch.Tensor:
    """One training-mode conv1x1 + BatchNormAct2d stage on the stage
    Function; the BN module's bookkeeping is done here as its forward does."""
    bn.num_batches_tracked += 1
    w, b = bn.weight, bn.bias
    if w.dtype != torch.float32:
        w, b = w.float(), b.float()
    return _PwConvBnActFn.apply(x, conv.weight, w, b, bn.running_mean,
                                bn.running_var, bn.momentum, bn.eps,
                                _ACT[bn.act])


def inverted_residual_train_fusable(block, x: torch.Tensor) -> bool:
    """The conditions under which a training-mode block takes the stage
    Function for its pointwise stages: mirrors
    ``inverted_residual_eval_fusable`` (CUDA bf16 input, fp32 BN buffers,
    the switches of ``conv.pw_train_enabled``, all read at call time)."""
    from .conv import pw_train_enabled

    if not block.training:
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return False
    if not pw_train_enabled():
        return False
    return all(_bn_fp32(bn) for _, bn in _stages(block))


def inverted_residual_train_forward(block, x: torch.Tensor) -> torch.Tensor:
    """Expand and project stages on the stage Function, the depthwise conv
    and its BN on their modules, the residual add eager."""
    h = x
    for conv, bn in _stages(block):
        if conv.pw_trainable() and bn.training:
            h = pw_conv_bn_train(conv, bn, h)
        else:
            h = bn(conv(h))
    return x + h if block.use_res else h
