"""Eval-mode MobileNetV2 inverted residual on fused kernels — the MobileNetV2
counterpart of ``bottleneck_eval_forward`` in ``ops/block.py``.

In a frozen base every BN is a constant per-channel affine, so it rides the
epilogue of the conv before it: an expanded block is three kernels
(pointwise MFMA expand + ReLU6, depthwise + ReLU6, pointwise project +
residual) instead of conv / bn_apply pairs and an eager add. Fed a uint8
batch, the frozen stem (normalize, 3->32 conv, BN, ReLU6) is one kernel too.
A stride-1 expanded block whose shape ``binding.mbconv_fused_route`` accepts
is ONE kernel (``hip/mbconv_fused.hip``, ``DDLW_MBCONV_FUSED``): the hidden
tensor lives in LDS only.
A stride-2 expanded block (``binding.mbconv_fused_s2_route``,
``DDLW_MBCONV_S2``) and the ``t = 1`` block (``binding.dwpw_fused_route``,
``DDLW_MBCONV_T1``) have a kernel each in the same file.

A training-mode block (the fine-tuned suffix) runs its two pointwise stages on
``_PwConvBnActFn``: the conv kernel emits the BN statistics from its epilogue
and the backward runs on the pointwise dgrad and the split-K wgrad kernels.
Under ``DDLW_DW_TRAIN=1`` the depthwise stage between them runs on
``_DwConvBnActFn`` the same way, its stride-1 backward in one kernel.
A marked training stem fed a uint8 batch runs on ``_StemU8BnActFn`` the same
way, its forward and its weight gradient reading the bytes.
A trainable block under FROZEN BatchNorms (``fine_tune_bn="frozen"``) runs on
``_PwConvFrozenBnActFn`` / ``_DwConvFrozenBnActFn``: folded forward kernels,
gated backward kernels (``DDLW_FROZEN_BN``).
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


def conv_bn_gap_eval(conv, bn, x: torch.Tensor) -> torch.Tensor:
    """A frozen conv + BatchNormAct2d stage whose only reader is the global
    average pool, as [N, K] pooled features: one kernel
    (``hip/pointwise_gap.hip``) when ``binding.pw_gap_route`` takes the shape
    (``DDLW_TAIL_GAP``), else ``conv_bn_eval`` and ``binding.gap_fwd``. The
    two are bit-equal."""
    n, _, h, w = x.shape
    if (_is_pointwise(conv) and conv.weight.dtype == torch.bfloat16
            and binding.pw_gap_route(conv.in_channels, conv.out_channels, h * w, n)):
        scale, bias = bn.folded_scale_bias()
        return binding.pw_conv_gap_fwd(x, conv.weight, scale, bias, _ACT[bn.act])
    y = conv_bn_eval(conv, bn, x)
    return binding.gap_fwd(y.contiguous(memory_format=torch.channels_last))


def _dw_w_t_cached(conv) -> torch.Tensor:
    """``binding._depthwise_w_t(conv.weight)`` ([9][C], tap-major), cached on
    the module until the weight mutates or moves (as ``_stem3_packed``)."""
    w = conv.weight
    key = (w._version, w.data_ptr(), w.device)
    cached = getattr(conv, "_dw_w_t_cache", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    w_t = binding._depthwise_w_t(w)
    conv._dw_w_t_cache = (key, w_t)
    return w_t


def _fused_block_stages(block, x: torch.Tensor):
    """The (expand, depthwise, project) stages of a frozen block that takes
    a one-kernel path (``hip/mbconv_fused.hip``), else ``None``: three
    stages pointwise / depthwise 3x3 pad 1 / pointwise with bf16 weights,
    ReLU6 after the first two BNs and none after the third, and a shape that
    ``binding.mbconv_fused_route`` (stride 1, ``DDLW_MBCONV_FUSED``) or
    ``binding.mbconv_fused_s2_route`` (stride 2, ``DDLW_MBCONV_S2``) accepts."""
    stages = _stages(block)
    if len(stages) != 3:
        return None
    (c1, n1), (c2, n2), (c3, n3) = stages
    if not (_is_pointwise(c1) and _is_pointwise(c3) and _is_depthwise3x3(c2)):
        return None
    if (n1.act, n2.act, n3.act) != ("relu6", "relu6", "none"):
        return None
    if any(c.weight.dtype != torch.bfloat16 for c in (c1, c2, c3)):
        return None
    chans = (c1.in_channels, c1.out_channels, c3.out_channels)
    if c2.stride == (2, 2):
        rows = x.shape[0] * ((x.shape[2] - 1) // 2 + 1) * ((x.shape[3] - 1) // 2 + 1)
        return stages if binding.mbconv_fused_s2_route(*chans, rows) else None
    rows = x.shape[0] * x.shape[2] * x.shape[3]
    return stages if binding.mbconv_fused_route(*chans, rows) else None


def _fused_t1_stages(block, x: torch.Tensor):
    """The (depthwise, project) stages of a frozen ``t = 1`` block that takes
    ``k_dwpw_fused``, else ``None``: depthwise 3x3 stride 1 pad 1 + ReLU6,
    pointwise with no activation, bf16 weights, and a shape
    ``binding.dwpw_fused_route`` accepts (``DDLW_MBCONV_T1``)."""
    stages = _stages(block)
    if len(stages) != 2:
        return None
    (c2, n2), (c3, n3) = stages
    if not (_is_depthwise3x3(c2) and c2.stride == (1, 1) and _is_pointwise(c3)):
        return None
    if (n2.act, n3.act) != ("relu6", "none"):
        return None
    if any(c.weight.dtype != torch.bfloat16 for c in (c2, c3)):
        return None
    rows = x.shape[0] * x.shape[2] * x.shape[3]
    if not binding.dwpw_fused_route(c3.in_channels, c3.out_channels, rows):
        return None
    return stages


@torch.no_grad()
def inverted_residual_eval_forward(block, x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous(memory_format=torch.channels_last)
    fused = _fused_block_stages(block, x)
    if fused is not None:
        (c1, n1), (c2, n2), (c3, n3) = fused
        args = (x, c1.weight, *n1.folded_scale_bias(), _dw_w_t_cached(c2),
                *n2.folded_scale_bias(), c3.weight, *n3.folded_scale_bias())
        if c2.stride == (2, 2):
            return binding.mbconv_fused_s2_fwd(*args)
        return binding.mbconv_fused_fwd(*args, block.use_res)
    fused = _fused_t1_stages(block, x)
    if fused is not None:
        (c2, n2), (c3, n3) = fused
        return binding.dwpw_fused_fwd(
            x, _dw_w_t_cached(c2), *n2.folded_scale_bias(), c3.weight,
            *n3.folded_scale_bias(), block.use_res)
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
        if (binding.pw_train_route("fwd", c, k, rows)
                or binding.pw_deep_route(c, k, rows) is not None):
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


# --------------------------------------------------------------------------- #
# Training-mode block: depthwise conv + BatchNorm stage on one Function
# --------------------------------------------------------------------------- #

# Off by default, by the project's rule (docs/KERNELS.md, "Depthwise conv +
# BN, training path"): at batch 64 / 224 the ``fine_tune_at=13`` step ran
# 1.03x the speed of ``DDLW_DW_TRAIN=0`` on medians in two runs, by more than
# that contender's spread in one of them (0.151 vs 0.123 ms) and inside it in
# the other (0.156 vs 0.225 ms).
_DW_TRAIN_DEFAULT = "0"


def dw_train_enabled() -> bool:
    """The A/B switch of the depthwise training stage, read at call time:
    ``DDLW_DW_TRAIN=1`` puts the depthwise conv + BN of a fusable training
    block on ``_DwConvBnActFn``, ``0`` (the default, see above) leaves them
    on their modules."""
    return os.environ.get("DDLW_DW_TRAIN", _DW_TRAIN_DEFAULT) != "0"


class _DwConvBnActFn(torch.autograd.Function):
    """depthwise conv3x3 -> BatchNormAct2d of a training-mode block; mirrors
    ``_PwConvBnActFn``. Forward: the depthwise kernel writes the conv output
    and its BN statistics partials in one pass. Backward: BN reduce, then at
    stride 1 one kernel for BN dx + dgrad + wgrad (``depthwise_bwd_bn``, no
    dz tensor); at stride 2, or when the weight wants no gradient, the three
    separate kernels, each only as needed. ``binding.dw_train_route`` sends
    the shapes that did not win by the measurement rule (the forward of the
    small, launch-bound layers) back to the kernels it replaces."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var,
                momentum: float, eps: float, act: int, stride: int, padding: int):
        x = x.contiguous(memory_format=torch.channels_last)
        c = weight.shape[0]
        ho = (x.shape[2] + 2 * padding - 3) // stride + 1
        wo = (x.shape[3] + 2 * padding - 3) // stride + 1
        rows = x.shape[0] * ho * wo
        if binding.dw_train_route("fwd", c, stride, rows):
            y, ps, pq, nparts = binding.depthwise_fwd_stats(x, weight, stride, padding)
            mean, rstd = binding.bn_finalize_parts(
                ps, pq, nparts, rows, c, eps, momentum, running_mean, running_var)
        else:
            y = binding.depthwise_fwd(x, weight, stride, padding)
            mean, rstd = binding.bn_stats(y, eps, momentum, running_mean,
                                          running_var)
        out, mask = binding.bn_apply(y, None, mean, rstd, gamma, beta, act)
        if mask is None:
            mask = x.new_empty(0, dtype=torch.uint8)
        ctx.save_for_backward(x, weight, y, mask, mean, rstd, gamma)
        ctx.relu = bool(act)  # the mask bit means "gradient passes"
        ctx.stride, ctx.padding = stride, padding
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, y, mask, mean, rstd, gamma = ctx.saved_tensors
        dout = dout.contiguous(memory_format=torch.channels_last)
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dbeta, dgamma = binding.bn_bwd_reduce(dout, mask, y, mean, rstd, ctx.relu)
        dx = dw = None
        rows = y.shape[0] * y.shape[2] * y.shape[3]
        if (need_dw and ctx.padding == 1
                and binding.dw_train_route("bwd", weight.shape[0], ctx.stride, rows)):
            dx, dw = binding.depthwise_bwd_bn(dout, mask, y, x, weight, mean, rstd,
                                              gamma, dbeta, dgamma, ctx.relu, need_dx)
        elif need_dx or need_dw:
            dz, _ = binding.bn_bwd_dx(dout, mask, y, mean, rstd, gamma, dbeta,
                                      dgamma, ctx.relu, False)
            if need_dx:
                dx = binding.depthwise_dgrad(dz, weight, x.shape, ctx.stride,
                                             ctx.padding)
            if need_dw:
                dw = binding.depthwise_wgrad(dz, x, weight.shape, ctx.stride,
                                             ctx.padding)
        if dw is not None:
            dw = dw.to(weight.dtype)
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None, None


def dw_conv_bn_train(conv, bn, x: torch.Tensor) -> torch.Tensor:
    """One training-mode depthwise conv3x3 + BatchNormAct2d stage on the
    stage Function; the BN module's bookkeeping is done here as its forward
    does."""
    bn.num_batches_tracked += 1
    w, b = bn.weight, bn.bias
    if w.dtype != torch.float32:
        w, b = w.float(), b.float()
    return _DwConvBnActFn.apply(x, conv.weight, w, b, bn.running_mean,
                                bn.running_var, bn.momentum, bn.eps,
                                _ACT[bn.act], conv.stride[0], conv.padding[0])


def _dw_trainable(conv) -> bool:
    return (_is_depthwise3x3(conv) and conv.weight.dtype == torch.bfloat16
            and dw_train_enabled())


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
    and its BN on theirs under ``DDLW_DW_TRAIN=1`` (else on their modules),
    the residual add eager."""
    h = x
    for conv, bn in _stages(block):
        if conv.pw_trainable() and bn.training:
            h = pw_conv_bn_train(conv, bn, h)
        elif bn.training and _dw_trainable(conv):
            h = dw_conv_bn_train(conv, bn, h)
        else:
            h = bn(conv(h))
    return x + h if block.use_res else h


# --------------------------------------------------------------------------- #
# Fine-tuned block with FROZEN BatchNorm: folded forward, gated backward
# --------------------------------------------------------------------------- #
#
# ``fine_tune_bn="frozen"`` (models/mobilenet_v2.py): the BatchNorms of the
# trainable suffix stay in eval mode with no-grad gamma / beta (the
# ``FrozenBatchNorm2d`` convention: a constant per-channel affine; NOT Keras's
# trainable gamma / beta under ``training=False``), only the conv weights
# train. A stage is then ``out = act(scale[k] * conv(x, W) + bias[k] (+ res))``
# on the folded forward kernels, and its whole BN + ReLU6 backward is
#   g16 = gate(out) ? bf16(fp32(dout) * scale[k]) : 0,  gate = 0 < out < 6,
# formed inside the conv's backward kernels (hip/pointwise_frozen.hip,
# k_depthwise_bwd_gated): no reductions, no dz tensor, no mask tensor.


def _gated_grad(dout, out, scale, act: int) -> torch.Tensor:
    """g16 as a tensor, for a direction ``binding.frozen_bn_route`` keeps on
    the kernels the gated ones replace."""
    g = (dout.float() * scale.view(1, -1, 1, 1)).to(torch.bfloat16)
    if act == 2:
        g = g * ((out > 0) & (out < 6))
    return g.contiguous(memory_format=torch.channels_last)


def _bf16_cl(dout: torch.Tensor) -> torch.Tensor:
    dout = dout.contiguous(memory_format=torch.channels_last)
    return dout if dout.dtype == torch.bfloat16 else dout.to(torch.bfloat16)


class _ResJoin:
    """The gradient that joins at a block's input through the residual: the
    project stage's backward leaves the block's ``dout`` here and the expand
    stage's dgrad adds it in its epilogue (``acc``), so the eager ``x + h``
    backward add is gone. The expand stage's backward runs after the project
    stage's: its gradient depends on it."""

    def __init__(self):
        self.dout = None


class _PwConvFrozenBnActFn(torch.autograd.Function):
    """conv1x1 -> frozen BatchNormAct2d (+ residual). Forward: the folded
    pointwise kernel. Backward: the gated dgrad / wgrad kernels, each only
    when needed. ``join`` is a ``_ResJoin``: a stage with ``res`` fills it
    (``res`` itself gets no gradient from here), a stage without takes its
    ``acc`` from it."""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, act: int, res, join):
        x = x.contiguous(memory_format=torch.channels_last)
        out = binding.pw_conv_fwd(x, weight, scale, bias, act, res)
        ctx.save_for_backward(x, weight, out, scale)
        ctx.act, ctx.join, ctx.fills = act, join, res is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        from .conv import pw_conv_backward

        x, weight, out, scale = ctx.saved_tensors
        dout = _bf16_cl(dout)
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        acc = None
        if ctx.join is not None:
            if ctx.fills:
                ctx.join.dout = dout
            else:
                acc, ctx.join.dout = ctx.join.dout, None
        k, c = weight.shape[0], weight.shape[1]
        rows = x.shape[0] * x.shape[2] * x.shape[3]
        fast_dx = need_dx and binding.frozen_bn_route("pw_dgrad", c, k, 1, rows)
        fast_dw = need_dw and binding.frozen_bn_route("pw_wgrad", c, k, 1, rows)
        dx = dw = None
        if fast_dx:
            dx = binding.pw_dgrad_gated(dout, out, weight, scale, ctx.act, x.shape, acc)
        if fast_dw:
            dw = binding.pw_wgrad_gated(dout, out, x, scale, ctx.act,
                                        weight.shape).to(weight.dtype)
        if (need_dx and not fast_dx) or (need_dw and not fast_dw):
            g = _gated_grad(dout, out, scale, ctx.act)
            gx, gw = pw_conv_backward(g, x, weight, need_dx and not fast_dx,
                                      need_dw and not fast_dw)
            if gx is not None:
                dx = gx if acc is None else gx + acc
            if gw is not None:
                dw = gw
        return dx, dw, None, None, None, None, None


class _DwConvFrozenBnActFn(torch.autograd.Function):
    """depthwise conv3x3 (pad 1, stride 1 or 2) -> frozen BatchNormAct2d.
    Forward: the folded depthwise kernel. Backward: one gated kernel for dx
    and dW."""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, act: int, stride: int):
        x = x.contiguous(memory_format=torch.channels_last)
        out = binding.depthwise_fwd_ep(x, weight, scale, bias, act, stride, 1)
        ctx.save_for_backward(x, weight, out, scale)
        ctx.act, ctx.stride = act, stride
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out, scale = ctx.saved_tensors
        dout = _bf16_cl(dout)
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        c = weight.shape[0]
        rows = out.shape[0] * out.shape[2] * out.shape[3]
        dx = dw = None
        if binding.frozen_bn_route("dw_bwd", c, c, ctx.stride, rows):
            dx, dw = binding.depthwise_bwd_gated(dout, out, x, weight, scale,
                                                 ctx.act, ctx.stride, need_dx)
        else:
            g = _gated_grad(dout, out, scale, ctx.act)
            if need_dx:
                dx = binding.depthwise_dgrad(g, weight, x.shape, ctx.stride, 1)
            if need_dw:
                dw = binding.depthwise_wgrad(g, x, weight.shape, ctx.stride, 1)
        if dw is not None:
            dw = dw.to(weight.dtype) if need_dw else None
        return dx, dw, None, None, None, None


def _bn_frozen(bn) -> bool:
    return (not bn.training and _bn_fp32(bn)
            and not bn.weight.requires_grad and not bn.bias.requires_grad)


def _frozen_bn_env(x: torch.Tensor) -> bool:
    if not torch.is_grad_enabled():
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return False
    if os.environ.get("DDLW_DISABLE_HIP_OPS", "0") == "1":
        return False
    if os.environ.get("DDLW_CONV", "auto") == "stock":
        return False
    return os.environ.get("DDLW_FROZEN_BN", "")[:1] != "0"


def _frozen_stage_kind(conv, bn):
    """``"pw"`` / ``"dw"`` for a stage the frozen-BN Functions take."""
    if conv.weight.dtype != torch.bfloat16 or _ACT[bn.act] not in (0, 2):
        return None
    if _is_pointwise(conv) and binding.pw_gated_supported(conv.in_channels,
                                                          conv.out_channels):
        return "pw"
    if _is_depthwise3x3(conv):
        return "dw"
    return None


def _frozen_stage_routed(kind, conv, rows_in: int, rows_out: int) -> bool:
    """Does any direction of the stage run on a gated kernel?"""
    c, k = conv.in_channels, conv.out_channels
    if kind == "pw":
        return (binding.frozen_bn_route("pw_dgrad", c, k, 1, rows_in)
                or binding.frozen_bn_route("pw_wgrad", c, k, 1, rows_in))
    return binding.frozen_bn_route("dw_bwd", c, c, conv.stride[0], rows_out)


def conv_bn_frozen_fusable(conv, bn, x: torch.Tensor) -> bool:
    """One conv + BatchNormAct2d stage (the 320 -> 1280 tail) on the frozen-BN
    stage Function: the conditions of ``inverted_residual_frozen_bn_fusable``
    for a single stage."""
    if not (_frozen_bn_env(x) and _bn_frozen(bn)):
        return False
    kind = _frozen_stage_kind(conv, bn)
    if kind is None:
        return False
    rows = x.shape[0] * x.shape[2] * x.shape[3]
    s = conv.stride[0]
    rows_out = x.shape[0] * ((x.shape[2] - 1) // s + 1) * ((x.shape[3] - 1) // s + 1)
    return _frozen_stage_routed(kind, conv, rows, rows_out)


def conv_bn_frozen(conv, bn, x: torch.Tensor, res=None, join=None) -> torch.Tensor:
    """One stage on its frozen-BN Function (the caller checked
    ``_frozen_stage_kind``)."""
    scale, bias = bn.folded_scale_bias()
    act = _ACT[bn.act]
    if _is_pointwise(conv):
        return _PwConvFrozenBnActFn.apply(x, conv.weight, scale, bias, act, res, join)
    return _DwConvFrozenBnActFn.apply(x, conv.weight, scale, bias, act, conv.stride[0])


def inverted_residual_frozen_bn_fusable(block, x: torch.Tensor) -> bool:
    """The conditions under which a block of the trainable suffix takes the
    frozen-BN stage Functions: grad enabled, every BN of the block in eval
    mode with fp32 buffers and no-grad parameters, bf16 conv weights of the
    pointwise / depthwise 3x3 shapes the gated kernels take, CUDA bf16 input,
    neither ``DDLW_DISABLE_HIP_OPS=1`` nor ``DDLW_CONV=stock``, and
    ``DDLW_FROZEN_BN`` (``0`` never, ``1`` always, unset: some direction of
    some stage is a measured winner, ``binding.frozen_bn_route``). All read
    at call time."""
    if not _frozen_bn_env(x) or x.dim() != 4:
        return False
    stages = _stages(block)
    if not all(_bn_frozen(bn) for _, bn in stages):
        return False
    kinds = [_frozen_stage_kind(conv, bn) for conv, bn in stages]
    if any(k is None for k in kinds):
        return False
    n, _, h, w = x.shape
    routed = False
    for kind, (conv, _) in zip(kinds, stages):
        s = conv.stride[0]
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        routed = routed or _frozen_stage_routed(kind, conv, n * h * w, n * ho * wo)
        h, w = ho, wo
    return routed


def inverted_residual_frozen_bn_forward(block, x: torch.Tensor) -> torch.Tensor:
    """Every stage on its frozen-BN Function. The residual rides the project
    stage's forward epilogue, and its gradient (the block's ``dout``) rides
    the expand stage's dgrad epilogue as ``acc`` (``_ResJoin``) when the
    input wants a gradient at all; a residual block whose first stage is not
    pointwise keeps the eager add."""
    stages = _stages(block)
    x = x.contiguous(memory_format=torch.channels_last)
    fused_res = (block.use_res and _is_pointwise(stages[-1][0])
                 and (not x.requires_grad
                      or (len(stages) == 3 and _is_pointwise(stages[0][0]))))
    join = _ResJoin() if (fused_res and x.requires_grad) else None
    h = x
    for i, (conv, bn) in enumerate(stages):
        last = i == len(stages) - 1
        if _is_pointwise(conv):
            h = conv_bn_frozen(conv, bn, h, res=x.detach() if (fused_res and last) else None,
                               join=join if (i == 0 or last) else None)
        else:
            h = conv_bn_frozen(conv, bn, h)
    if block.use_res and not fused_res:
        return x + h
    return h
