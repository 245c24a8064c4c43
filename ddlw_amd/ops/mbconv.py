"""Eval-mode MobileNetV2 inverted residual on fused kernels — the MobileNetV2
counterpart of ``bottleneck_eval_forward`` in ``ops/block.py``.

In a frozen base every BN is a constant per-channel affine, so it rides the
epilogue of the conv before it: an expanded block is three kernels
(pointwise MFMA expand + ReLU6, depthwise + ReLU6, pointwise project +
residual) instead of conv / bn_apply pairs and an eager add.
"""
from __future__ import annotations

import os

import torch

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
