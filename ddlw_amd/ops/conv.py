"""Conv2d with dispatch between the ddlw MFMA implicit-GEMM HIP kernels and
the library path (MIOpen via F.conv2d).

The reference's convolutions live behind TF/Keras (kernels K1-K3 in
SURVEY.md §2.4); here they are first-class. Dispatch policy via
``DDLW_CONV`` env: ``auto`` (default — per-shape pick from the measured
table), ``hip`` (force hand-written kernels), ``stock`` (force MIOpen).
"""
from __future__ import annotations

import os
import torch
import torch.nn as nn
import torch.nn.functional as F


def conv_mode() -> str:
    return os.environ.get("DDLW_CONV", "auto")


class _DepthwiseFn(torch.autograd.Function):
    """Depthwise 3x3 conv (K2) with hand-written backward: forward is the
    existing ``binding.depthwise_fwd``; backward launches the dgrad and
    wgrad kernels, each only when its gradient is needed."""

    @staticmethod
    def forward(ctx, x, weight, stride: int, padding: int):
        from . import binding

        x = x.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.padding = stride, padding
        return binding.depthwise_fwd(x, weight, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        from . import binding

        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        if dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = binding.depthwise_dgrad(dy, weight, x.shape, ctx.stride,
                                         ctx.padding)
        if ctx.needs_input_grad[1]:
            dw = binding.depthwise_wgrad(dy, x, weight.shape, ctx.stride,
                                         ctx.padding).to(weight.dtype)
        return dx, dw, None, None


def pw_train_enabled() -> bool:
    """The switches of the pointwise training route, read at call time:
    ``DDLW_PW_TRAIN`` (default ``1``; ``0`` = the library path, for A/B),
    ``DDLW_CONV=stock`` and ``DDLW_DISABLE_HIP_OPS=1``."""
    return (os.environ.get("DDLW_PW_TRAIN", "1") != "0"
            and conv_mode() != "stock"
            and os.environ.get("DDLW_DISABLE_HIP_OPS", "0") != "1")


def pw_conv_backward(dy, x, weight, need_dx: bool, need_dw: bool):
    """(dx, dw) of a 1x1 stride-1 conv, each only when needed and each on
    our kernel or the library as ``binding.pw_train_route`` says."""
    from . import binding

    dy = dy.contiguous(memory_format=torch.channels_last)
    if dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)
    k, c = weight.shape[0], weight.shape[1]
    rows = x.shape[0] * x.shape[2] * x.shape[3]
    dx = dw = None
    lib_dx = need_dx and not binding.pw_train_route("dgrad", c, k, rows)
    lib_dw = need_dw and not binding.pw_train_route("wgrad", c, k, rows)
    if need_dx and not lib_dx:
        dx = binding.pw_conv_dgrad(dy, weight, x.shape)
    if need_dw and not lib_dw:
        dw = binding.pw_conv_wgrad(dy, x, weight.shape).to(weight.dtype)
    if lib_dx or lib_dw:
        gi, gw, _ = torch.ops.aten.convolution_backward(
            dy, x, weight.to(dy.dtype), None, [1, 1], [0, 0], [1, 1], False,
            [0, 0], 1, [lib_dx, lib_dw, False])
        if lib_dx:
            dx = gi
        if lib_dw:
            dw = gw.to(weight.dtype)
    return dx, dw


class _PointwiseFn(torch.autograd.Function):
    """Trainable 1x1 stride-1 conv — the counterpart of ``_DepthwiseFn``:
    forward on the pointwise MFMA kernel, backward the same kernel on
    (dy, w^T) for dgrad and the split-K wgrad kernel, each only when its
    gradient is needed."""

    @staticmethod
    def forward(ctx, x, weight):
        from . import binding

        x = x.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x, weight)
        k, c = weight.shape[0], weight.shape[1]
        rows = x.shape[0] * x.shape[2] * x.shape[3]
        if binding.pw_train_route("fwd", c, k, rows):
            return binding.pw_conv_train_fwd(x, weight)
        return F.conv2d(x, weight.to(x.dtype))

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        return pw_conv_backward(dy, x, weight, ctx.needs_input_grad[0],
                                ctx.needs_input_grad[1])


class Conv2d(nn.Conv2d):
    """nn.Conv2d subclass so init/state_dict/bias handling are inherited;
    forward dispatches per policy. HIP implicit-GEMM path: ops.conv_gemm.

    ``pw_train``: opt-in mark a model sets on its 1x1 convs (an instance
    attribute, not a parameter or buffer) to train them on the pointwise
    MFMA kernels; unmarked convs keep the routing below.

    ``u8_train``: the same kind of mark on a MobileNetV2 stem conv
    (``MobileNetV2.enable_u8_train_stem``): a training stem takes a uint8
    batch on the fused stem kernels (``ops/mbconv.py``). This forward never
    reads it."""

    pw_train = False
    u8_train = False

    def pw_trainable(self) -> bool:
        """A marked 1x1 stride-1 pad-0 conv of a shape the pointwise
        kernels take."""
        return (self.pw_train
                and self.kernel_size == (1, 1) and self.stride == (1, 1)
                and self.padding == (0, 0) and self.dilation == (1, 1)
                and self.groups == 1 and self.bias is None
                and self.in_channels % 8 == 0 and self.out_channels % 8 == 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        mode = conv_mode()
        hip_ok = (
            mode != "stock"
            and x.is_cuda
            and x.dtype == torch.bfloat16
            and self.dilation == (1, 1)
            and os.environ.get("DDLW_DISABLE_HIP_OPS", "0") != "1"
        )
        if (
            hip_ok
            and self.groups == self.in_channels == self.out_channels
            and self.in_channels % 8 == 0
            and self.bias is None
            and (
                not torch.is_grad_enabled()  # inference: fwd-only kernel safe
                or not (x.requires_grad or self.weight.requires_grad)
            )
        ):
            # depthwise (K2 — MobileNetV2 blocks), inference/frozen path
            from . import binding

            st = self.stride[0] if isinstance(self.stride, tuple) else self.stride
            pd = self.padding[0] if isinstance(self.padding, tuple) else self.padding
            return binding.depthwise_fwd(
                x.contiguous(memory_format=torch.channels_last), self.weight, st, pd
            )
        if (
            hip_ok
            and self.groups == self.in_channels == self.out_channels
            and self.in_channels % 8 == 0
            and self.bias is None
            and self.kernel_size == (3, 3)
            and self.stride in ((1, 1), (2, 2))
            and isinstance(self.padding, tuple)
            and self.padding[0] == self.padding[1]
        ):
            # depthwise, trainable path: fwd kernel + dgrad/wgrad kernels
            return _DepthwiseFn.apply(
                x, self.weight, self.stride[0], self.padding[0]
            )
        if (
            hip_ok
            and self.pw_trainable()
            and torch.is_grad_enabled()
            and (x.requires_grad or self.weight.requires_grad)
            and pw_train_enabled()
        ):
            # opted-in pointwise conv, trainable path (no-grad calls fall
            # through to the routing below, as before)
            return _PointwiseFn.apply(x, self.weight)
        if (
            hip_ok
            and self.groups == 1
            and self.in_channels == 3
            and self.out_channels == 64
            and self.kernel_size == (7, 7)
            and self.stride == (2, 2)
            and self.padding == (3, 3)
            and self.bias is None
            and os.environ.get("DDLW_STEM", "1") == "1"
        ):
            # dedicated C=3 stem kernel (K1): c4+halo repack + 2x8x4 igemm
            from . import conv_gemm

            return conv_gemm.stem_conv2d(x, self.weight)
        if hip_ok and self.groups == 1:
            from . import conv_gemm

            if conv_gemm.available(self, x, mode):
                hip_fwd, hip_dgrad, hip_wgrad = self._ddlw_route
                return conv_gemm.conv2d(
                    x, self.weight, self.bias, self.stride, self.padding,
                    hip_fwd, hip_dgrad, hip_wgrad,
                )
        return F.conv2d(
            x, self.weight.to(x.dtype),
            None if self.bias is None else self.bias.to(x.dtype),
            self.stride, self.padding, self.dilation, self.groups,
        )
