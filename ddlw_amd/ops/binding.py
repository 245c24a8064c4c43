"""Tensor-level wrappers over libddlw_kernels.so (ABI: ``abi.py``).

All activation tensors must be channels_last (NHWC memory) bf16; statistics
and parameters fp32. Every call launches onto torch's current HIP stream, so
the kernels are stream-ordered with PyTorch ops and hipGraph-capturable.
"""
from __future__ import annotations

import functools
import os
from typing import Optional

import torch

from .runtime import launch, query


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """A channels_last bf16 activation (N,C,H,W logical), checked."""
    if t.dim() == 4:
        assert t.is_contiguous(memory_format=torch.channels_last), "need channels_last"
    else:
        assert t.is_contiguous()
    assert t.dtype == torch.bfloat16, f"need bf16, got {t.dtype}"
    return t


def _rows_c(t: torch.Tensor):
    if t.dim() == 4:
        n, c, h, w = t.shape
        return n * h * w, c
    rows, c = t.shape[0], t.shape[-1]
    return rows, c


def supported_channels(c: int) -> bool:
    return c % 8 == 0


@functools.lru_cache(maxsize=512)
def _nparts(rows: int, C: int) -> int:
    return int(query("bn_nparts", rows, C))


def bn_stats(x: torch.Tensor, eps: float, momentum: float,
             running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor]):
    rows, C = _rows_c(x)
    dev = x.device
    ny = _nparts(rows, C)
    part = torch.empty(2, ny, C, dtype=torch.float32, device=dev)
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    launch("bn_stats", _nhwc(x), part[0], part[1], rows, C)
    launch("bn_finalize", part[0], part[1], mean, rstd, running_mean,
           running_var, rows, C, ny, eps, momentum)
    return mean, rstd


def _fold_parts(p0: torch.Tensor, p1: torch.Tensor, nparts: int, C: int):
    """Pre-reduce a large pair of [nparts, C] partial arrays to G rows with a
    chip-filling grid: the finalize kernels run ceil(C/32) blocks and would
    serialize a 12k-row partial read on 2 CUs."""
    if nparts <= 512:
        return p0, p1, nparts
    G = max(8, 512 // max(1, (C + 31) // 32))
    stage = torch.empty(2, G, C, dtype=torch.float32, device=p0.device)
    launch("bn_parts_fold", p0, p1, stage[0], stage[1], nparts, C, G)
    return stage[0], stage[1], G


def bn_finalize_parts(part_sum: torch.Tensor, part_sumsq: torch.Tensor,
                      nparts: int, rows: int, C: int, eps: float,
                      momentum: float, running_mean, running_var):
    """Finalize mean/rstd from conv-epilogue-fused partial sums (the
    k_bn_stats read pass is skipped entirely)."""
    dev = part_sum.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    part_sum, part_sumsq, nparts = _fold_parts(part_sum, part_sumsq, nparts, C)
    launch("bn_finalize", part_sum, part_sumsq, mean, rstd, running_mean,
           running_var, rows, C, nparts, eps, momentum)
    return mean, rstd


def bn_grad_finalize_parts(part_db: torch.Tensor, part_dg: torch.Tensor,
                           nparts: int, C: int):
    """(dbeta, dgamma) from dgrad-epilogue-fused reduce partials."""
    dev = part_db.device
    part_db, part_dg, nparts = _fold_parts(part_db, part_dg, nparts, C)
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    launch("bn_grad_finalize", part_db, part_dg, dbeta, dgamma, C, nparts)
    return dbeta, dgamma


def bn_apply(x: torch.Tensor, res: Optional[torch.Tensor], mean, rstd, gamma, beta,
             relu):
    """Returns (y, mask): mask is a uint8 tensor of rows*C/8 relu bits (one
    byte per 8-channel vector) when relu, else None — backward reads the
    mask instead of re-reading y.

    ``relu``: False/0 = identity, True/1 = ReLU, 2 = ReLU6. A mask bit means
    "gradient passes here" (``0 < f < 6`` for ReLU6), so the backward
    kernels take a ReLU6 layer as ``relu=True``."""
    relu = int(relu)
    if relu not in (0, 1, 2):
        raise ValueError(f"bn_apply: relu mode must be 0, 1 or 2, got {relu}")
    rows, C = _rows_c(x)
    y = torch.empty_like(x)
    mask = (
        torch.empty(rows * (C // 8), dtype=torch.uint8, device=x.device)
        if relu
        else None
    )
    launch("bn_apply", _nhwc(x), res, _nhwc(y), mask, mean, rstd, gamma, beta,
           rows, C, relu)
    return y, mask


def bn_bwd_reduce(dy, mask, x, mean, rstd, relu: bool):
    rows, C = _rows_c(x)
    dev = x.device
    ny = _nparts(rows, C)
    part = torch.empty(2, ny, C, dtype=torch.float32, device=dev)
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    launch("bn_bwd_reduce", _nhwc(dy), mask, _nhwc(x), mean, rstd, part[0],
           part[1], rows, C, 1 if relu else 0)
    launch("bn_grad_finalize", part[0], part[1], dbeta, dgamma, C, ny)
    return dbeta, dgamma


def bn_bwd_dx(dy, mask, x, mean, rstd, gamma, dbeta, dgamma, relu: bool,
              want_dres: bool):
    rows, C = _rows_c(x)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    launch("bn_bwd_dx", _nhwc(dy), mask, _nhwc(x), mean, rstd, gamma, dbeta,
           dgamma, dx, dres, rows, C, 1 if relu else 0)
    return dx, dres


def maxpool3x3s2_fwd(x: torch.Tensor):
    n, c, h, w = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    y = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device,
                    memory_format=torch.channels_last)
    argmax = torch.empty(n * ho * wo * c, dtype=torch.uint8, device=x.device)
    launch("maxpool3x3s2_fwd", _nhwc(x), _nhwc(y), argmax, n, h, w, c, ho, wo)
    return y, argmax


def maxpool3x3s2_bwd(dy: torch.Tensor, argmax: torch.Tensor, in_shape):
    n, c, h, w = in_shape
    ho, wo = dy.shape[2], dy.shape[3]
    dx = torch.empty((n, c, h, w), dtype=dy.dtype, device=dy.device,
                     memory_format=torch.channels_last)
    launch("maxpool3x3s2_bwd", _nhwc(dy), argmax, _nhwc(dx), n, h, w, c, ho, wo)
    return dx


def gap_fwd(x: torch.Tensor) -> torch.Tensor:
    n, c, h, w = x.shape
    y = torch.empty((n, c), dtype=x.dtype, device=x.device)
    launch("gap_fwd", _nhwc(x), y, n, h * w, c)
    return y


def gap_bwd(dy: torch.Tensor, in_shape) -> torch.Tensor:
    n, c, h, w = in_shape
    dx = torch.empty((n, c, h, w), dtype=dy.dtype, device=dy.device,
                     memory_format=torch.channels_last)
    launch("gap_bwd", dy.contiguous(), _nhwc(dx), n, h * w, c)
    return dx


def softmax_ce(logits: torch.Tensor, labels: torch.Tensor, grad_scale: float):
    """Returns (mean loss tensor [1], dlogits). logits fp32 [B,K]."""
    B, K = logits.shape
    logits = logits.contiguous()
    dlogits = torch.empty_like(logits)
    loss_sum = torch.zeros(1, dtype=torch.float32, device=logits.device)
    launch("softmax_ce", logits, labels.contiguous(), dlogits, loss_sum, B, K,
           grad_scale)
    return loss_sum / B, dlogits


@functools.lru_cache(maxsize=512)
def ce_metrics_nblocks(B: int, K: int) -> int:
    """Blocks ``ce_metrics`` walks [B, K] logits with: 1 is the single
    launch, more is the rows kernel plus its finalize."""
    return int(query("ce_metrics_nblocks", B, K, None))


def ce_metrics(logits: torch.Tensor, labels: torch.Tensor, grad_scale: float,
               accum: Optional[torch.Tensor] = None, want_grad: bool = True):
    """Loss, gradient and metrics of one step from the logits in one pass.
    logits [B, K] bf16 or fp32, labels [B] (cast to int64). Returns
    ``(step_out, dlogits)``: ``step_out`` fp32 [2] = (mean loss, accuracy);
    ``dlogits`` = ``(softmax - onehot) * grad_scale`` in the logits' dtype,
    ``None`` without ``want_grad``. ``accum``: fp64 [4] on the logits'
    device, updated in place: += (mean loss, accuracy, 1, bad labels). A
    label outside [0, K) gives zero loss and gradient and is counted there."""
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"ce_metrics: logits must be bf16 or fp32, got {logits.dtype}")
    assert logits.dim() == 2, "ce_metrics: logits must be [B, K]"
    B, K = logits.shape
    assert labels.numel() == B, f"ce_metrics: {labels.numel()} labels for {B} rows"
    assert labels.device == logits.device, "ce_metrics: labels on another device"
    logits = logits.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.to(torch.int64)
    labels = labels.contiguous()
    if accum is not None:
        assert (accum.dtype == torch.float64 and accum.is_contiguous()
                and accum.numel() == 4 and accum.device == logits.device), \
            "ce_metrics: accum must be a contiguous fp64 [4] on the logits' device"
    dev = logits.device
    dlogits = torch.empty_like(logits) if want_grad else None
    step_out = torch.empty(2, dtype=torch.float32, device=dev)
    nb = ce_metrics_nblocks(B, K) if B > 0 and K > 0 else 1
    part = torch.empty(3 * nb, dtype=torch.int32, device=dev) if nb > 1 else None
    launch("ce_metrics", logits, labels, dlogits, step_out, accum, part, B, K,
           grad_scale, 1 if logits.dtype == torch.bfloat16 else 0)
    return step_out, dlogits


def fused_sgd(chunk_desc: torch.Tensor, nchunks: int, max_numel: int, lr: float,
              momentum: float, weight_decay: float, first_step: bool):
    """chunk_desc: int64 device tensor [nchunks, 5] of
    (p_ptr, g_ptr, m_ptr, p_bf16_ptr_or_0, numel)."""
    launch("fused_sgd", chunk_desc, nchunks, max_numel, lr, momentum,
           weight_decay, 1 if first_step else 0)


def normalize_u8(x_u8: torch.Tensor, out_bf16: torch.Tensor):
    n = x_u8.numel()
    assert n % 16 == 0
    launch("normalize_u8", x_u8, out_bf16, n)


def fused_adam(chunk_desc: torch.Tensor, nchunks: int, max_numel: int,
               lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, bc1: float, bc2: float):
    """chunk_desc: int64 device tensor [nchunks, 7] of
    (p_ptr, g_ptr, m_ptr, v_ptr, p_bf16_ptr_or_0, numel, flags)."""
    launch("fused_adam", chunk_desc, nchunks, max_numel, lr, beta1, beta2, eps,
           weight_decay, bc1, bc2)


def fused_adadelta(chunk_desc: torch.Tensor, nchunks: int, max_numel: int,
                   lr: float, rho: float, eps: float, weight_decay: float):
    """chunk_desc: int64 device tensor [nchunks, 7] of
    (p_ptr, g_ptr, square_avg_ptr, acc_delta_ptr, p_bf16_ptr_or_0, numel,
    flags)."""
    launch("fused_adadelta", chunk_desc, nchunks, max_numel, lr, rho, eps,
           weight_decay)


def _depthwise_w_t(weight: torch.Tensor) -> torch.Tensor:
    """weight [C,1,R,S] -> bf16 [R*S][C], so taps read contiguous channel
    vectors."""
    c, _, r, s = weight.shape
    w_t = weight.detach().reshape(c, r * s).t().contiguous()
    if w_t.dtype != torch.bfloat16:
        w_t = w_t.to(torch.bfloat16)
    return w_t


def depthwise_fwd(x: torch.Tensor, weight: torch.Tensor, stride: int, padding: int) -> torch.Tensor:
    """Depthwise conv2d forward (groups == C), weight [C,1,R,S]."""
    n, c, h, w = x.shape
    _, _, r, s = weight.shape
    ho = (h + 2 * padding - r) // stride + 1
    wo = (w + 2 * padding - s) // stride + 1
    y = torch.empty((n, c, ho, wo), dtype=torch.bfloat16, device=x.device,
                    memory_format=torch.channels_last)
    launch("depthwise_fwd", _nhwc(x), _depthwise_w_t(weight), _nhwc(y),
           n, h, w, c, ho, wo, r, s, stride, padding)
    return y


def _f32c(t: torch.Tensor, c: int) -> torch.Tensor:
    """A contiguous fp32 per-channel vector of length ``c``, checked."""
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == c
    return t


def depthwise_fwd_ep(x: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor,
                     bias: torch.Tensor, act: int, stride: int,
                     padding: int) -> torch.Tensor:
    """Depthwise 3x3 forward with the folded-BN epilogue:
    ``act(dw(x) * scale[c] + bias[c])``, act 0 none / 1 ReLU / 2 ReLU6.
    scale and bias fp32 [C]; weight [C,1,3,3]."""
    n, c, h, w = x.shape
    _, _, r, s = weight.shape
    assert (r, s) == (3, 3), "depthwise_fwd_ep is 3x3 only"
    ho = (h + 2 * padding - r) // stride + 1
    wo = (w + 2 * padding - s) // stride + 1
    y = torch.empty((n, c, ho, wo), dtype=torch.bfloat16, device=x.device,
                    memory_format=torch.channels_last)
    launch("depthwise_fwd_ep", _nhwc(x), _depthwise_w_t(weight), _nhwc(y),
           _f32c(scale, c), _f32c(bias, c), int(act), n, h, w, c, ho, wo,
           stride, padding)
    return y


def pw_conv_supported(C: int, K: int) -> bool:
    """Shapes ``pw_conv_fwd`` takes: 16-byte bf16x8 vectors on both channel
    axes. No measured-loser exclusion: every pointwise shape of MobileNetV2
    @224 beat the unfused path by more than its spread
    (bench/bench_mobilenet.py; table and rule in docs/KERNELS.md)."""
    return C > 0 and K > 0 and C % 8 == 0 and K % 8 == 0


def pw_conv_fwd(x: torch.Tensor, weight: torch.Tensor,
                scale: Optional[torch.Tensor] = None,
                bias: Optional[torch.Tensor] = None, act: int = 0,
                res: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1x1 stride-1 conv on the MFMA pointwise kernel with its epilogue:
    ``act(conv(x) * scale[k] + bias[k] + res)``. x channels_last bf16
    [N,C,H,W] (or rows [M,C]); weight [K,C,1,1] (or [K,C]); scale/bias fp32
    [K], both or neither; res like the output; act 0 none / 1 ReLU / 2 ReLU6.
    ``out``: write into this bf16 tensor of the output's shape and layout."""
    K, C = weight.shape[0], weight.shape[1]
    rows, cx = _rows_c(x)
    assert cx == C, f"pw_conv_fwd: x has {cx} channels, weight {C}"
    if not pw_conv_supported(C, K):
        raise ValueError(f"pw_conv_fwd: C={C}, K={K} must be multiples of 8")
    w2 = weight.detach().reshape(K, C)
    if w2.dtype != torch.bfloat16:
        w2 = w2.to(torch.bfloat16)
    w2 = w2.contiguous()
    if x.dim() == 4:
        n, _, h, w_ = x.shape
        shape = (n, K, h, w_)
    else:
        shape = (rows, K)
    if out is not None:
        assert tuple(out.shape) == shape, "pw_conv_fwd: out has the wrong shape"
        y = _nhwc(out)
    elif x.dim() == 4:
        y = torch.empty(shape, dtype=torch.bfloat16, device=x.device,
                        memory_format=torch.channels_last)
    else:
        y = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    if res is not None:
        assert res.shape == y.shape, "pw_conv_fwd: res must match the output"
        res = _nhwc(res)
    if scale is not None:
        scale, bias = _f32c(scale, K), _f32c(bias, K)
    launch("pw_conv_fwd", _nhwc(x), w2, y, res, scale, bias, int(act), rows, C,
           K)
    return y


# ---- MobileNetV2 stem from uint8 ------------------------------------------- #


def stem3_pack_weight(weight: torch.Tensor) -> torch.Tensor:
    """weight [K,C,3,3] -> bf16 [K][32] for ``stem3_u8_fwd_ep``: row k holds
    ``w[k][r][s][c]`` at ``9r + 3s + c`` (a window row is 9 contiguous input
    bytes) and zeros from 9*C = 27 up: the 27-deep reduction as one 32-deep
    MFMA step."""
    K, C, r, s = weight.shape
    assert (r, s) == (3, 3), "stem3_pack_weight: 3x3 only"
    cols = -(-r * s * C // 32) * 32
    wp = torch.zeros(K, cols, dtype=torch.bfloat16, device=weight.device)
    wp[:, : r * s * C] = weight.detach().permute(0, 2, 3, 1).reshape(K, r * s * C)
    return wp


def stem3_u8_fwd_ep(x_u8: torch.Tensor, weight: torch.Tensor,
                    scale: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, act: int = 0,
                    wp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The MobileNetV2 stem on a uint8 image batch in one kernel:
    ``act(conv3x3_s2_p1(x/127.5 - 1) * scale[k] + bias[k])`` with the
    normalized input rounded to bf16 as ``normalize_u8_bf16`` does. x_u8
    uint8 [N,3,H,W] channels_last (NHWC memory); weight [32,3,3,3]; scale/bias
    fp32 [32], both or neither; act 0 none / 1 ReLU / 2 ReLU6. Returns bf16
    [N,32,Ho,Wo] channels_last. ``wp``: ``stem3_pack_weight(weight)`` if the
    caller already holds it. Other shapes are the kernel library's to refuse."""
    assert x_u8.is_cuda and weight.device == x_u8.device, "stem3_u8_fwd_ep: need one GPU"
    assert x_u8.dtype == torch.uint8, f"stem3_u8_fwd_ep: need uint8, got {x_u8.dtype}"
    assert x_u8.dim() == 4 and x_u8.is_contiguous(memory_format=torch.channels_last), \
        "stem3_u8_fwd_ep: need a channels_last [N,C,H,W] batch"
    n, c, h, w = x_u8.shape
    K = weight.shape[0]
    assert weight.shape[1] == c, f"stem3_u8_fwd_ep: x has {c} channels, weight {weight.shape[1]}"
    if wp is None:
        wp = stem3_pack_weight(weight)
    assert (wp.dtype == torch.bfloat16 and wp.is_contiguous()
            and tuple(wp.shape) == (K, -(-9 * c // 32) * 32)), "stem3_u8_fwd_ep: wp"
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, K, ho, wo), dtype=torch.bfloat16, device=x_u8.device,
                    memory_format=torch.channels_last)
    if scale is not None and bias is not None:
        scale, bias = _f32c(scale, K), _f32c(bias, K)
    assert all(t is None or t.device == x_u8.device for t in (wp, scale, bias))
    launch("stem3_u8_fwd_ep", x_u8, wp, y, scale, bias, int(act), n, h, w, c, K)
    return y


@functools.lru_cache(maxsize=64)
def _stem3_u8_nparts(rows: int) -> int:
    return int(query("stem3_u8_nparts", rows, None))


@functools.lru_cache(maxsize=64)
def _stem3_u8_wgrad_nparts(rows: int) -> int:
    return int(query("stem3_u8_wgrad_nparts", rows, None))


def stem3_u8_fwd_stats(x_u8: torch.Tensor, weight: torch.Tensor,
                       wp: Optional[torch.Tensor] = None):
    """Training forward of the MobileNetV2 stem on a uint8 image batch:
    ``conv3x3_s2_p1(x/127.5 - 1)`` raw (no scale, bias or activation) with
    the BatchNorm statistics of its output from the epilogue. Returns ``(y,
    part_sum, part_sumsq, nparts)``: y bf16 [N,32,Ho,Wo] channels_last,
    bit-equal to ``stem3_u8_fwd_ep(x_u8, weight)``; the partials fp32
    ``[nparts, 32]``, sums over the bf16 ``y``, for ``bn_finalize_parts``.
    Arguments as ``stem3_u8_fwd_ep``'s."""
    assert x_u8.is_cuda and weight.device == x_u8.device, "stem3_u8_fwd_stats: need one GPU"
    assert x_u8.dtype == torch.uint8, f"stem3_u8_fwd_stats: need uint8, got {x_u8.dtype}"
    assert x_u8.dim() == 4 and x_u8.is_contiguous(memory_format=torch.channels_last), \
        "stem3_u8_fwd_stats: need a channels_last [N,C,H,W] batch"
    n, c, h, w = x_u8.shape
    K = weight.shape[0]
    assert weight.shape[1] == c, f"stem3_u8_fwd_stats: x has {c} channels, weight {weight.shape[1]}"
    if wp is None:
        wp = stem3_pack_weight(weight)
    assert (wp.dtype == torch.bfloat16 and wp.is_contiguous() and wp.device == x_u8.device
            and tuple(wp.shape) == (K, -(-9 * c // 32) * 32)), "stem3_u8_fwd_stats: wp"
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, K, ho, wo), dtype=torch.bfloat16, device=x_u8.device,
                    memory_format=torch.channels_last)
    nparts = _stem3_u8_nparts(n * ho * wo)
    both = torch.empty(2, max(nparts, 1), K, dtype=torch.float32, device=x_u8.device)
    ps, pq = both[0, :nparts], both[1, :nparts]
    launch("stem3_u8_fwd_stats", x_u8, wp, y, both[0], both[1], nparts, n, h, w, c, K)
    return y, ps, pq, nparts


def stem3_u8_wgrad(x_u8: torch.Tensor, dy: torch.Tensor, weight_shape) -> torch.Tensor:
    """Weight gradient of the MobileNetV2 stem from the uint8 image batch,
    fp32 [32,3,3,3]: ``dW[k][c][r][s] = sum dy[n][k][ho][wo] *
    xn[n][c][2ho-1+r][2wo-1+s]`` with ``xn`` the ``normalize_u8_bf16`` value
    gathered from the bytes (zero padding in normalized space). dy bf16
    [N,32,Ho,Wo] channels_last. Two launches (per-block partials, then a
    fixed-order sum): no atomics, bit-reproducible."""
    assert x_u8.is_cuda and dy.device == x_u8.device, "stem3_u8_wgrad: need one GPU"
    assert x_u8.dtype == torch.uint8, f"stem3_u8_wgrad: need uint8, got {x_u8.dtype}"
    assert x_u8.dim() == 4 and x_u8.is_contiguous(memory_format=torch.channels_last), \
        "stem3_u8_wgrad: need a channels_last [N,C,H,W] batch"
    n, c, h, w = x_u8.shape
    K, wc, r, s = weight_shape
    assert wc == c, f"stem3_u8_wgrad: x has {c} channels, weight {wc}"
    assert (r, s) == (3, 3), "stem3_u8_wgrad: 3x3 only"
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert tuple(dy.shape) == (n, K, ho, wo), \
        f"stem3_u8_wgrad: dy is {tuple(dy.shape)}, the output is {(n, K, ho, wo)}"
    nparts = _stem3_u8_wgrad_nparts(n * ho * wo)
    part = torch.empty(max(nparts, 1), K, r * s * c, dtype=torch.float32,
                       device=x_u8.device)
    dw = torch.empty((K, c, r, s), dtype=torch.float32, device=x_u8.device)
    launch("stem3_u8_wgrad", x_u8, _nhwc(dy), part, dw, nparts, n, h, w, c, K)
    return dw


# ---- pointwise conv, training path ---------------------------------------- #


def pw_train_route(direction: str, C: int, K: int, M: int) -> bool:
    """True: this direction (``"fwd"`` = forward + BN statistics, ``"dgrad"``,
    ``"wgrad"``) of an opted-in 1x1 conv C -> K over M rows runs on our
    kernel; False: on the library path it replaces. The one place where a
    measured loser is excluded (rule, table and verdicts:
    docs/KERNELS.md, "Pointwise conv, training path")."""
    if direction not in ("fwd", "dgrad", "wgrad"):
        raise ValueError(f"pw_train_route: unknown direction {direction!r}")
    if not pw_conv_supported(C, K):
        return False
    if os.environ.get("DDLW_CONV", "auto") == "hip":
        return True  # force the hand-written kernels, as for every other conv
    # The rows of the measured table (MobileNetV2 @224, batch 64) that did
    # not beat the library by more than its spread. A verdict holds from its
    # measured row count up; below it nothing is measured and the shape
    # stays on our kernel.
    if direction == "wgrad":
        # k_conv_wgrad's 64-wide tiles are mostly empty at 16 / 24 channels
        # and there are rows enough to show it: 0.89x, 0.97x, 0.92x
        if (C, K) == (32, 16) and M >= 802816:
            return False
        if (C, K) in ((24, 144), (144, 24)) and M >= 200704:
            return False
        return True
    # fwd and dgrad are the same GEMM; its loop is not software-pipelined,
    # so a 960- or 1280-deep reduction is 30 / 40 dependent load -> MFMA
    # steps, and at 3136 rows its 25-50 blocks leave most of the chip idle:
    # fwd 960->160 1.11x inside the spread, 960->320 1.00x; dgrad of
    # 160->960 0.72x, of 320->1280 0.56x. Up to one 128-row block per CU.
    depth = C if direction == "fwd" else K
    if depth >= 960 and 3136 <= M < 256 * 128:
        return False
    # 96->24 at 56x56: 1.16x, inside the library's spread
    if direction == "fwd" and (C, K) == (96, 24) and M >= 200704:
        return False
    return True


@functools.lru_cache(maxsize=512)
def _pw_conv_nparts(rows: int, K: int) -> int:
    return int(query("pw_conv_nparts", rows, K, None))


def _pw_w2(weight: torch.Tensor) -> torch.Tensor:
    """weight [K,C,1,1] (or [K,C]) -> contiguous bf16 [K][C]."""
    w2 = weight.detach().reshape(weight.shape[0], weight.shape[1])
    if w2.dtype != torch.bfloat16:
        w2 = w2.to(torch.bfloat16)
    return w2.contiguous()


def _pw_out(x: torch.Tensor, rows: int, K: int, out, who: str) -> torch.Tensor:
    """The [rows, K] output of a pointwise GEMM over ``x``: 4-D channels_last
    when x is, ``out`` itself when given."""
    shape = (x.shape[0], K, x.shape[2], x.shape[3]) if x.dim() == 4 else (rows, K)
    if out is not None:
        assert tuple(out.shape) == shape, f"{who}: out has the wrong shape"
        return _nhwc(out)
    if x.dim() == 4:
        return torch.empty(shape, dtype=torch.bfloat16, device=x.device,
                           memory_format=torch.channels_last)
    return torch.empty(shape, dtype=torch.bfloat16, device=x.device)


def _pw_gemm(x: torch.Tensor, w2: torch.Tensor, res, out, who: str) -> torch.Tensor:
    """``x [rows, C] * w2[K, C]^T (+ res)`` on the pointwise kernel with no
    affine and no activation."""
    K, C = w2.shape
    rows, cx = _rows_c(x)
    assert cx == C, f"{who}: input has {cx} channels, weights take {C}"
    if not pw_conv_supported(C, K):
        raise ValueError(f"{who}: C={C}, K={K} must be multiples of 8")
    y = _pw_out(x, rows, K, out, who)
    if res is not None:
        assert res.shape == y.shape, f"{who}: acc must match the output"
        res = _nhwc(res)
    launch("pw_conv_fwd", _nhwc(x), w2, y, res, None, None, 0, rows, C, K)
    return y


def pw_conv_train_fwd(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Training forward of a 1x1 stride-1 conv without statistics (a conv
    whose BatchNorm is not fused to it): ``conv(x)``, bf16."""
    return _pw_gemm(x, _pw_w2(weight), None, None, "pw_conv_train_fwd")


def pw_conv_fwd_stats(x: torch.Tensor, weight: torch.Tensor, parts=None):
    """Training forward of a 1x1 stride-1 conv with the BatchNorm statistics
    of its output from the epilogue: returns ``(y, part_sum, part_sumsq,
    nparts)`` with the partials fp32 ``[nparts, K]``, sums over the bf16
    ``y``, for ``bn_finalize_parts``. ``parts``: a pair of contiguous fp32
    ``[nparts, K]`` tensors to write into."""
    w2 = _pw_w2(weight)
    K, C = w2.shape
    rows, cx = _rows_c(x)
    assert cx == C, f"pw_conv_fwd_stats: x has {cx} channels, weight {C}"
    if not pw_conv_supported(C, K):
        raise ValueError(f"pw_conv_fwd_stats: C={C}, K={K} must be multiples of 8")
    nparts = _pw_conv_nparts(rows, K)
    if parts is None:
        both = torch.empty(2, nparts, K, dtype=torch.float32, device=x.device)
        ps, pq = both[0], both[1]
    else:
        ps, pq = parts
        for t in (ps, pq):
            assert (t.dtype == torch.float32 and t.is_contiguous()
                    and tuple(t.shape) == (nparts, K)), "pw_conv_fwd_stats: parts"
    y = _pw_out(x, rows, K, None, "pw_conv_fwd_stats")
    launch("pw_conv_fwd_stats", _nhwc(x), w2, y, ps, pq, rows, C, K)
    return y, ps, pq, nparts


def pw_conv_dgrad(dy: torch.Tensor, weight: torch.Tensor, in_shape,
                  acc: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None,
                  w_t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of a 1x1 stride-1 conv, ``dx[m][c] = sum_k dy[m][k] *
    w[k][c] (+ acc)``: the pointwise GEMM with dy as the rows and w^T as the
    weights. dy channels_last bf16 [N,K,H,W] (or rows [M,K]); weight
    [K,C,1,1]; returns dx of ``in_shape``. ``acc``: dx-shaped bf16 tensor
    added in the epilogue. ``w_t``: the bf16 [C][K] transpose if the caller
    already holds it (else rebuilt here: weights change every step)."""
    if w_t is None:
        w_t = _pw_w2(weight).t().contiguous()
    assert w_t.dtype == torch.bfloat16 and w_t.is_contiguous()
    dx = _pw_gemm(dy, w_t, acc, out, "pw_conv_dgrad")
    assert tuple(dx.shape) == tuple(in_shape), "pw_conv_dgrad: in_shape"
    return dx


def pw_conv_wgrad(dy: torch.Tensor, x: torch.Tensor, weight_shape) -> torch.Tensor:
    """Weight gradient of a 1x1 stride-1 conv, bf16 [K,C,1,1]: the split-K
    implicit-GEMM wgrad kernel at R = S = 1."""
    from . import conv_gemm

    return conv_gemm.conv_wgrad_kernel(dy, x, weight_shape, 1, 0)


def depthwise_dgrad(dy: torch.Tensor, weight: torch.Tensor, in_shape,
                    stride: int, padding: int) -> torch.Tensor:
    """Depthwise 3x3 conv2d input gradient. dy [N,C,Ho,Wo] channels_last
    bf16, weight [C,1,3,3]; returns dx of ``in_shape`` (N,C,H,W),
    channels_last bf16. Every dx element is written by the kernel."""
    n, c, h, w = in_shape
    _, _, r, s = weight.shape
    ho, wo = dy.shape[2], dy.shape[3]
    assert dy.shape[0] == n and dy.shape[1] == c == weight.shape[0]
    dx = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=dy.device,
                     memory_format=torch.channels_last)
    launch("depthwise_dgrad", _nhwc(dy), _depthwise_w_t(weight), _nhwc(dx),
           n, h, w, c, ho, wo, r, s, stride, padding)
    return dx


@functools.lru_cache(maxsize=512)
def _depthwise_wgrad_nparts(rows: int, C: int) -> int:
    return int(query("depthwise_wgrad_nparts", rows, C))


def depthwise_wgrad(dy: torch.Tensor, x: torch.Tensor, weight_shape,
                    stride: int, padding: int) -> torch.Tensor:
    """Depthwise 3x3 conv2d weight gradient, fp32 [C,1,3,3]. dy and x are
    channels_last bf16. Two launches (row-slice partials, then a fixed-order
    sum): no atomics, bit-reproducible."""
    n, c, h, w = x.shape
    _, _, r, s = weight_shape
    ho, wo = dy.shape[2], dy.shape[3]
    assert dy.shape[0] == n and dy.shape[1] == c == weight_shape[0]
    nparts = _depthwise_wgrad_nparts(n * ho * wo, c)
    part = torch.empty(nparts, r * s, c, dtype=torch.float32, device=x.device)
    dw = torch.empty((c, 1, r, s), dtype=torch.float32, device=x.device)
    launch("depthwise_wgrad", _nhwc(dy), _nhwc(x), part, dw,
           n, h, w, c, ho, wo, r, s, stride, padding)
    return dw


def dropout_fwd(x: torch.Tensor, p: float, seed: int):
    """K7: bitmask dropout (counter-based RNG, deterministic per seed).
    Returns (y, mask); x flat-size must be a multiple of 8."""
    n = x.numel()
    y = torch.empty_like(x)
    mask = torch.empty(n // 8, dtype=torch.uint8, device=x.device)
    launch("dropout_fwd", x, y, mask, n, p, seed & (2**64 - 1))
    return y, mask


def dropout_bwd(dy: torch.Tensor, mask: torch.Tensor, p: float):
    dx = torch.empty_like(dy)
    launch("dropout_bwd", dy, mask, dx, dy.numel(), p)
    return dx


def argmax_rows(logits: torch.Tensor) -> torch.Tensor:
    """K12: per-row argmax (first-max tie-break, like torch.argmax)."""
    lf = logits.float().contiguous()
    n, c = lf.shape
    out = torch.empty(n, dtype=torch.long, device=lf.device)
    launch("argmax_rows", lf, out, n, c)
    return out


def accuracy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """K11: mean(argmax(logits) == labels) via per-block partial counts."""
    lf = logits.float().contiguous()
    n, c = lf.shape
    nblocks = (n + 3) // 4
    partial = torch.empty(nblocks, dtype=torch.int32, device=lf.device)
    launch("accuracy", lf, labels.contiguous(), partial, n, c)
    return partial.sum().float() / n
