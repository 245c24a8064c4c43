"""The bf16 policy — the one state the hand-written kernels are gated on.

Every fused path (frozen MobileNetV2, uint8 stem, pointwise/depthwise
training, fused BN, fused optimizers) runs on a CUDA **bf16**, channels_last
input with bf16 conv/linear weights, plus a uint8 batch for the fused stem.
``apply_bf16_policy`` puts a module into that state, ``prepare_batch`` a batch;
``train.Model(precision="bf16")`` calls both.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .layers import normalize_u8_bf16


def apply_bf16_policy(module: nn.Module) -> nn.Module:
    """channels_last memory format, conv/linear weights (and biases) in bf16,
    BatchNorm parameters and buffers left in fp32 (the eval-BN fold and the
    fused BN kernels read them as fp32). A pure cast: ``Parameter`` objects
    and their ``requires_grad`` flags are kept (a ``fine_tune_at`` split
    survives), a second call changes nothing, and it works on a CPU module.
    Build optimizers AFTER it, so fp32 masters start from the cast weights.

    The policy is also the door to the opt-in kernel routes: a submodule with
    ``enable_u8_train_stem`` (MobileNetV2) gets its training stem marked for
    the uint8 stem kernels. The mark is an instance attribute, so it is not
    saved: a reloaded model is unmarked until the policy is applied again."""
    module = module.to(memory_format=torch.channels_last)
    for mod in module.modules():
        if isinstance(mod, (nn.Conv2d, nn.Linear)):
            mod.to(torch.bfloat16)
        if hasattr(mod, "enable_u8_train_stem"):
            mod.enable_u8_train_stem()
    return module


def _u8_nchw_view(x: torch.Tensor) -> torch.Tensor:
    """A 4-D uint8 batch as the N x C x H x W view over NHWC memory."""
    nhwc = x.is_contiguous() and x.shape[-1] <= 4
    nchw_cl = (x.is_contiguous(memory_format=torch.channels_last)
               and x.shape[1] <= 4)
    if nhwc and nchw_cl:
        raise ValueError(
            f"uint8 batch of shape {tuple(x.shape)} reads both as N x H x W x C "
            "and as channels_last N x C x H x W; pass an explicit layout (a "
            "float batch, or a shape whose channel dim is unambiguous)")
    if nhwc:
        return x.permute(0, 3, 1, 2)
    if nchw_cl:
        return x
    if x.shape[1] <= 4:
        return x.contiguous(memory_format=torch.channels_last)
    raise ValueError(
        f"uint8 batch of shape {tuple(x.shape)} (strides {x.stride()}) is "
        "neither N x H x W x C nor N x C x H x W with at most 4 channels")


def prepare_batch(module: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """A batch already on the device -> what a module under the bf16 policy
    takes. uint8 is the fast door: N x H x W x C as the loader yields it (or
    its channels_last N x C x H x W view) goes in as uint8 when the module
    sets ``accepts_uint8`` (its fused stem normalizes), else through
    ``normalize_u8_bf16``. A float 4-D batch is cast to bf16 channels_last in
    torch ops; any other rank is cast to bf16."""
    if x.dtype == torch.uint8:
        if x.dim() != 4:
            raise ValueError(f"uint8 batches must be 4-D images, got {tuple(x.shape)}")
        x = _u8_nchw_view(x)
        if getattr(module, "accepts_uint8", False):
            return x
        return normalize_u8_bf16(x)
    if x.dim() == 4:
        return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return x.to(torch.bfloat16)
