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

from .runtime import TICKET_INTS, launch, query, ticket_buffer


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


_FOLD_ABOVE = 512  # partial rows the finalize kernels take directly


def _fold_groups(C: int) -> int:
    """Stage rows G a large partial set is folded to: a chip-filling grid of
    (ceil(C/32), G) blocks."""
    return max(8, 512 // max(1, (C + 31) // 32))


def _fold_parts(p0: torch.Tensor, p1: torch.Tensor, nparts: int, C: int):
    """Pre-reduce a large pair of [nparts, C] partial arrays to G rows with a
    chip-filling grid: the finalize kernels run ceil(C/32) blocks and would
    serialize a 12k-row partial read on 2 CUs."""
    if nparts <= _FOLD_ABOVE:
        return p0, p1, nparts
    G = _fold_groups(C)
    stage = torch.empty(2, G, C, dtype=torch.float32, device=p0.device)
    launch("bn_parts_fold", p0, p1, stage[0], stage[1], nparts, C, G)
    return stage[0], stage[1], G


def bn_folded_enabled() -> bool:
    """``DDLW_BN_FOLDED``, read per call: ``1`` -> a partial set of more than
    512 rows is folded and finalized in one launch (``hip/bn_folded.hip``);
    unset / ``0`` -> ``k_bn_parts_fold`` and the finalize kernel, two
    launches. The results are bit-identical either way. Off by default: a
    measured loss on the flagship (docs/KERNELS.md, "Measured negative
    results")."""
    return os.environ.get("DDLW_BN_FOLDED", "")[:1] == "1"


def _folded_args(p0: torch.Tensor, nparts: int, C: int):
    """(stage [2, G, C], ticket buffer, its length, G) of a folded finalize,
    or None where the two-launch path runs."""
    if (nparts <= _FOLD_ABOVE or (C + 31) // 32 > TICKET_INTS
            or not bn_folded_enabled()):
        return None
    G = _fold_groups(C)
    stage = torch.empty(2, G, C, dtype=torch.float32, device=p0.device)
    ticket = ticket_buffer(p0.device)
    return stage, ticket, ticket.numel(), G


def bn_finalize_parts(part_sum: torch.Tensor, part_sumsq: torch.Tensor,
                      nparts: int, rows: int, C: int, eps: float,
                      momentum: float, running_mean, running_var):
    """Finalize mean/rstd from conv-epilogue-fused partial sums (the
    k_bn_stats read pass is skipped entirely)."""
    dev = part_sum.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    folded = _folded_args(part_sum, nparts, C)
    if folded is not None:
        stage, ticket, nticket, G = folded
        launch("bn_finalize_folded", part_sum, part_sumsq, stage, ticket,
               nticket, mean, rstd, running_mean, running_var, rows, C,
               nparts, G, eps, momentum)
        return mean, rstd
    part_sum, part_sumsq, nparts = _fold_parts(part_sum, part_sumsq, nparts, C)
    launch("bn_finalize", part_sum, part_sumsq, mean, rstd, running_mean,
           running_var, rows, C, nparts, eps, momentum)
    return mean, rstd


def bn_grad_finalize_parts(part_db: torch.Tensor, part_dg: torch.Tensor,
                           nparts: int, C: int):
    """(dbeta, dgamma) from dgrad-epilogue-fused reduce partials."""
    dev = part_db.device
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    folded = _folded_args(part_db, nparts, C)
    if folded is not None:
        stage, ticket, nticket, G = folded
        launch("bn_grad_finalize_folded", part_db, part_dg, stage, ticket,
               nticket, dbeta, dgamma, C, nparts, G)
        return dbeta, dgamma
    part_db, part_dg, nparts = _fold_parts(part_db, part_dg, nparts, C)
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
    ``out``: write into this bf16 tensor of the output's shape and layout.
    A shape ``pw_deep_route`` names runs on the split-reduction kernel."""
    rows, _ = _rows_c(x)
    return _pw_conv_fwd(x, weight, scale, bias, act, res, out,
                        pw_deep_route(weight.shape[1], weight.shape[0], rows))


def pw_conv_deep_fwd(x: torch.Tensor, weight: torch.Tensor,
                     scale: Optional[torch.Tensor] = None,
                     bias: Optional[torch.Tensor] = None, act: int = 0,
                     res: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None,
                     mr: Optional[int] = None) -> torch.Tensor:
    """``pw_conv_fwd`` on the split-reduction kernel (``hip/pointwise_deep.hip``)
    whatever the route says: same arguments, same result shape. ``mr``: 1 or 2
    16-row fragments per block tile; ``None`` takes the route's choice, else 2."""
    rows, _ = _rows_c(x)
    return _pw_conv_fwd(x, weight, scale, bias, act, res, out,
                        _pw_deep_mr(mr, weight.shape[1], weight.shape[0], rows))


def _pw_conv_fwd(x, weight, scale, bias, act, res, out, mr) -> torch.Tensor:
    """``pw_conv_fwd`` on the plain kernel (``mr`` None) or the
    split-reduction one with ``mr`` fragments per tile."""
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
    if mr is None:
        launch("pw_conv_fwd", _nhwc(x), w2, y, res, scale, bias, int(act), rows,
               C, K)
    else:
        launch("pw_conv_deep_fwd", _nhwc(x), w2, y, res, scale, bias, int(act),
               rows, C, K, mr)
    return y


# ---- frozen inverted residual in one kernel -------------------------------- #

_MBF_MAX_CIN, _MBF_MAX_COUT = 160, 320


def mbconv_fused_supported(Cin: int, Chid: int, Cout: int, stride: int = 1) -> bool:
    """Shapes ``mbconv_fused_fwd`` takes: stride 1, 16-byte bf16x8 vectors on
    the three channel axes, an x tile (``Cin <= 160``) and project
    accumulators (``Cout <= 320``) that fit LDS and registers."""
    return (stride == 1 and min(Cin, Chid, Cout) > 0
            and Cin % 8 == 0 and Chid % 8 == 0 and Cout % 8 == 0
            and Cin <= _MBF_MAX_CIN and Cout <= _MBF_MAX_COUT)


# (Cin, Chid, Cout) -> (smallest, largest) measured row count N*H*W of the
# --only-mbconv-fused table (bench/bench_mobilenet.py) whose median beat the
# three-kernel path by more than that path's spread, at batch 16, 64 and 256
# alike (the bounds are the batch-16 and batch-256 row counts; the speedups
# are those three batches in order). No measured loser: a shape that loses a
# later measurement leaves this table and is named here with its figures.
_MBCONV_FUSED_MEASURED = {
    (24, 144, 24): (50176, 802816),    # 56x56: 1.78x, 1.14x, 1.25x
    (32, 192, 32): (12544, 200704),    # 28x28: 1.78x, 1.85x, 1.40x
    (64, 384, 64): (3136, 50176),      # 14x14: 1.77x, 1.87x, 1.70x
    (64, 384, 96): (3136, 50176),      # 14x14: 1.78x, 1.87x, 1.75x
    (96, 576, 96): (3136, 50176),      # 14x14: 1.84x, 1.89x, 1.59x
    (160, 960, 160): (784, 12544),     # 7x7, N workgroups only: 1.29x, 1.29x, 1.50x
    (160, 960, 320): (784, 12544),     # 7x7: 1.09x, 1.09x, 1.26x
}


def mbconv_fused_route(Cin: int, Chid: int, Cout: int, rows: int) -> bool:
    """True: a frozen stride-1 expand / depthwise 3x3 / project block over
    ``rows`` = N*H*W pixels runs on the one-kernel path
    (``hip/mbconv_fused.hip``); False: on the three kernels it replaces.
    ``DDLW_MBCONV_FUSED``, read per call: ``0`` -> never; ``1`` -> every
    supported shape; unset -> the measured winners only, each within its
    measured row range (table and rule: docs/KERNELS.md, "mbconv_fused.hip")."""
    if rows <= 0 or not mbconv_fused_supported(Cin, Chid, Cout, 1):
        return False
    mode = os.environ.get("DDLW_MBCONV_FUSED", "")[:1]
    if mode == "0":
        return False
    if mode == "1":
        return True
    row = _MBCONV_FUSED_MEASURED.get((Cin, Chid, Cout))
    return row is not None and row[0] <= rows <= row[1]


def mbconv_fused_fwd(x: torch.Tensor, w1: torch.Tensor, s1: torch.Tensor,
                     b1: torch.Tensor, wd: torch.Tensor, s2: torch.Tensor,
                     b2: torch.Tensor, w3: torch.Tensor, s3: torch.Tensor,
                     b3: torch.Tensor, res: bool,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A frozen stride-1 inverted residual in one launch:
    ``relu6(x*w1^T*s1+b1)`` -> ``relu6(dw3x3(.)*s2+b2)`` -> ``(.)*w3^T*s3+b3``
    ``(+ x)``, the two hidden tensors rounded to bf16 as the three-kernel path
    rounds them. x channels_last bf16 [N,Cin,H,W]; w1 [Chid,Cin,1,1] or
    [Chid,Cin]; wd [9,Chid] (tap-major, what ``_depthwise_w_t`` gives) or the
    conv's [Chid,1,3,3]; w3 [Cout,Chid,1,1] or [Cout,Chid]; s*/b* the folded
    BN, fp32; ``res`` adds x (``Cin == Cout``). ``out``: write into this bf16
    channels_last tensor [N,Cout,H,W]."""
    who = "mbconv_fused_fwd"
    if x.dim() != 4:
        raise ValueError(f"{who}: x must be [N,C,H,W], got {tuple(x.shape)}")
    n, cin, h, w = x.shape
    if w1.dim() not in (2, 4) or w3.dim() not in (2, 4):
        raise ValueError(f"{who}: w1 / w3 must be 2-D or 1x1 4-D")
    chid, cout = w1.shape[0], w3.shape[0]
    if tuple(w1.shape[1:]) not in ((cin,), (cin, 1, 1)):
        raise ValueError(f"{who}: w1 is {tuple(w1.shape)}, x has {cin} channels")
    if tuple(w3.shape[1:]) not in ((chid,), (chid, 1, 1)):
        raise ValueError(f"{who}: w3 is {tuple(w3.shape)}, hidden width {chid}")
    if not mbconv_fused_supported(cin, chid, cout, 1):
        raise ValueError(
            f"{who}: Cin={cin}, Chid={chid}, Cout={cout} must be multiples of 8"
            f" with Cin <= {_MBF_MAX_CIN} and Cout <= {_MBF_MAX_COUT}")
    if res and cin != cout:
        raise ValueError(f"{who}: the residual needs Cin == Cout, got {cin}, {cout}")
    if tuple(wd.shape) == (chid, 1, 3, 3):
        wd = _depthwise_w_t(wd)
    elif tuple(wd.shape) != (9, chid):
        raise ValueError(f"{who}: wd is {tuple(wd.shape)}, want (9, {chid})")
    for name, t in (("x", x), ("w1", w1), ("wd", wd), ("w3", w3)):
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{who}: {name} must be bf16, got {t.dtype}")
    for name, t, c in (("s1", s1, chid), ("b1", b1, chid), ("s2", s2, chid),
                       ("b2", b2, chid), ("s3", s3, cout), ("b3", b3, cout)):
        if t.dtype != torch.float32 or t.numel() != c or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous fp32 [{c}], got "
                             f"{t.dtype} {tuple(t.shape)}")
    y = _pw_out(x, n * h * w, cout, out, who)
    launch("mbconv_fused_fwd", _nhwc(x), _pw_w2(w1), s1, b1, wd.contiguous(),
           s2, b2, _pw_w2(w3), s3, b3, y, n, h, w, cin, chid, cout, int(bool(res)))
    return y


# ---- frozen stride-2 block and t = 1 block in one kernel each --------------- #

_MBF_S2_MAX_CIN, _DWPW_MAX_C = 96, 64


def _route_mode(switch: str, measured: dict, key, rows: int) -> bool:
    """``0`` -> never; ``1`` -> always; unset -> ``key`` is a measured winner
    and ``rows`` lies in its measured range. Read per call."""
    mode = os.environ.get(switch, "")[:1]
    if mode == "0":
        return False
    if mode == "1":
        return True
    row = measured.get(key)
    return row is not None and row[0] <= rows <= row[1]


def _fused_block_args(who, x, wd, chid, named_bf16, folds):
    """The argument checks the one-kernel blocks share: bf16 operands, fp32
    contiguous folds, ``wd`` as [9, Chid] or the conv's [Chid, 1, 3, 3]
    (returned tap-major)."""
    if tuple(wd.shape) == (chid, 1, 3, 3):
        wd = _depthwise_w_t(wd)
    elif tuple(wd.shape) != (9, chid):
        raise ValueError(f"{who}: wd is {tuple(wd.shape)}, want (9, {chid})")
    for name, t in (("x", x), ("wd", wd), *named_bf16):
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{who}: {name} must be bf16, got {t.dtype}")
    for name, t, c in folds:
        if t.dtype != torch.float32 or t.numel() != c or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous fp32 [{c}], got "
                             f"{t.dtype} {tuple(t.shape)}")
    return wd.contiguous()


def _fused_block_out(who, x, shape, out):
    if out is not None:
        if tuple(out.shape) != shape:
            raise ValueError(f"{who}: out is {tuple(out.shape)}, want {shape}")
        return _nhwc(out)
    return torch.empty(shape, dtype=torch.bfloat16, device=x.device,
                       memory_format=torch.channels_last)


def mbconv_fused_s2_supported(Cin: int, Chid: int, Cout: int) -> bool:
    """Shapes ``mbconv_fused_s2_fwd`` takes: 16-byte bf16x8 vectors on the
    three channel axes, ``Cin <= 96`` (the x halo, ``h1`` and ``h2`` within
    64 KB of LDS) and ``Cout <= 320``."""
    return (min(Cin, Chid, Cout) > 0
            and Cin % 8 == 0 and Chid % 8 == 0 and Cout % 8 == 0
            and Cin <= _MBF_S2_MAX_CIN and Cout <= _MBF_MAX_COUT)


# (Cin, Chid, Cout) -> (smallest, largest) measured OUTPUT row count N*Ho*Wo
# (batch 16 and batch 256 at 224^2) of the stride-2 rows of the
# --only-mbconv-fused table (bench/bench_mobilenet.py) whose median beat the
# three-kernel path by more than that path's spread at batch 16, 64 and 256
# alike, in every run (rule and figures: docs/KERNELS.md, "k_mbconv_fused_s2";
# the speedups are those three batches in order, two runs). No measured loser:
# a shape that loses a later measurement leaves this table and is named here
# with its figures.
_MBCONV_S2_MEASURED = {
    (16, 96, 24): (50176, 802816),     # 112->56: 1.82-1.84x, 1.12-1.13x, 1.45x
    (24, 144, 32): (12544, 200704),    # 56->28: 1.79-1.82x, 1.79-1.81x, 1.57-1.58x
    (32, 192, 64): (3136, 50176),      # 28->14: 1.82-1.84x, 1.84-1.85x, 1.81-1.83x
    (96, 576, 160): (784, 12544),      # 14->7: 1.85-1.86x, 1.84-1.86x, 1.18-1.20x
}


def mbconv_fused_s2_route(Cin: int, Chid: int, Cout: int, rows: int) -> bool:
    """True: a frozen expand / depthwise 3x3 stride 2 / project block with
    ``rows`` = N*Ho*Wo OUTPUT pixels runs on ``k_mbconv_fused_s2``; False: on
    the three kernels it replaces. ``DDLW_MBCONV_S2``, read per call: ``0`` ->
    never; ``1`` -> every supported shape; unset -> the measured winners only,
    each within its measured row range."""
    if rows <= 0 or not mbconv_fused_s2_supported(Cin, Chid, Cout):
        return False
    return _route_mode("DDLW_MBCONV_S2", _MBCONV_S2_MEASURED, (Cin, Chid, Cout), rows)


def mbconv_fused_s2_fwd(x: torch.Tensor, w1: torch.Tensor, s1: torch.Tensor,
                        b1: torch.Tensor, wd: torch.Tensor, s2: torch.Tensor,
                        b2: torch.Tensor, w3: torch.Tensor, s3: torch.Tensor,
                        b3: torch.Tensor,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A frozen stride-2 inverted residual in one launch: the function of
    ``mbconv_fused_fwd`` with a stride-2 pad-1 depthwise and no residual, same
    operands. Returns (or writes into ``out``) bf16 channels_last
    [N, Cout, (H-1)//2+1, (W-1)//2+1]."""
    who = "mbconv_fused_s2_fwd"
    if x.dim() != 4:
        raise ValueError(f"{who}: x must be [N,C,H,W], got {tuple(x.shape)}")
    n, cin, h, w = x.shape
    if w1.dim() not in (2, 4) or w3.dim() not in (2, 4):
        raise ValueError(f"{who}: w1 / w3 must be 2-D or 1x1 4-D")
    chid, cout = w1.shape[0], w3.shape[0]
    if tuple(w1.shape[1:]) not in ((cin,), (cin, 1, 1)):
        raise ValueError(f"{who}: w1 is {tuple(w1.shape)}, x has {cin} channels")
    if tuple(w3.shape[1:]) not in ((chid,), (chid, 1, 1)):
        raise ValueError(f"{who}: w3 is {tuple(w3.shape)}, hidden width {chid}")
    if not mbconv_fused_s2_supported(cin, chid, cout):
        raise ValueError(
            f"{who}: Cin={cin}, Chid={chid}, Cout={cout} must be multiples of 8"
            f" with Cin <= {_MBF_S2_MAX_CIN} and Cout <= {_MBF_MAX_COUT}")
    wd = _fused_block_args(who, x, wd, chid, (("w1", w1), ("w3", w3)),
                           (("s1", s1, chid), ("b1", b1, chid), ("s2", s2, chid),
                            ("b2", b2, chid), ("s3", s3, cout), ("b3", b3, cout)))
    y = _fused_block_out(who, x, (n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), out)
    launch("mbconv_fused_s2_fwd", _nhwc(x), _pw_w2(w1), s1, b1, wd, s2, b2,
           _pw_w2(w3), s3, b3, y, n, h, w, cin, chid, cout)
    return y


def dwpw_fused_supported(C: int, Cout: int) -> bool:
    """Shapes ``dwpw_fused_fwd`` takes: multiples of 8, both at most 64 (one
    chunk of channels, at most two output pairs)."""
    return (min(C, Cout) > 0 and C % 8 == 0 and Cout % 8 == 0
            and C <= _DWPW_MAX_C and Cout <= _DWPW_MAX_C)


# (C, Cout) -> (smallest, largest) measured row count N*H*W, as above, for the
# t = 1 block (docs/KERNELS.md, "k_dwpw_fused"). No measured loser.
_DWPW_MEASURED = {
    (32, 16): (200704, 3211264),       # 112x112: 1.61-1.66x, 1.39-1.40x, 1.44x
}


def dwpw_fused_route(C: int, Cout: int, rows: int) -> bool:
    """True: a frozen ``t = 1`` block (depthwise 3x3 stride 1 / project) over
    ``rows`` = N*H*W pixels runs on ``k_dwpw_fused``; False: on the two
    kernels it replaces. ``DDLW_MBCONV_T1``, read per call, as
    ``mbconv_fused_s2_route`` reads its switch."""
    if rows <= 0 or not dwpw_fused_supported(C, Cout):
        return False
    return _route_mode("DDLW_MBCONV_T1", _DWPW_MEASURED, (C, Cout), rows)


def dwpw_fused_fwd(x: torch.Tensor, wd: torch.Tensor, s2: torch.Tensor,
                   b2: torch.Tensor, w3: torch.Tensor, s3: torch.Tensor,
                   b3: torch.Tensor, res: bool,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A frozen ``t = 1`` inverted residual in one launch:
    ``relu6(dw3x3(x)*s2+b2)`` (stride 1, pad 1, rounded to bf16 as
    ``depthwise_fwd_ep`` rounds it) -> ``(.)*w3^T*s3+b3 (+ x)``. x
    channels_last bf16 [N,C,H,W]; wd [9,C] (tap-major) or the conv's
    [C,1,3,3]; w3 [Cout,C,1,1] or [Cout,C]; s*/b* the folded BN, fp32;
    ``res`` adds x (``C == Cout``). ``out``: write into this bf16
    channels_last tensor [N,Cout,H,W]."""
    who = "dwpw_fused_fwd"
    if x.dim() != 4:
        raise ValueError(f"{who}: x must be [N,C,H,W], got {tuple(x.shape)}")
    n, c, h, w = x.shape
    if w3.dim() not in (2, 4) or tuple(w3.shape[1:]) not in ((c,), (c, 1, 1)):
        raise ValueError(f"{who}: w3 is {tuple(w3.shape)}, x has {c} channels")
    cout = w3.shape[0]
    if not dwpw_fused_supported(c, cout):
        raise ValueError(f"{who}: C={c}, Cout={cout} must be multiples of 8, at"
                         f" most {_DWPW_MAX_C}")
    if res and c != cout:
        raise ValueError(f"{who}: the residual needs C == Cout, got {c}, {cout}")
    wd = _fused_block_args(who, x, wd, c, (("w3", w3),),
                           (("s2", s2, c), ("b2", b2, c), ("s3", s3, cout),
                            ("b3", b3, cout)))
    y = _fused_block_out(who, x, (n, cout, h, w), out)
    launch("dwpw_fused_fwd", _nhwc(x), wd, s2, b2, _pw_w2(w3), s3, b3, y, n, h, w,
           c, cout, int(bool(res)))
    return y


# ---- frozen tail: pointwise conv + BN + activation + GAP in one kernel ------- #

_PW_GAP_MAX_C = 320


def pw_conv_gap_supported(C: int, K: int) -> bool:
    """Shapes ``pw_conv_gap_fwd`` takes: 16-byte bf16x8 vectors on both
    channel axes and a weight slab that fits the registers (``C <= 320``)."""
    return 8 <= C <= _PW_GAP_MAX_C and K > 0 and C % 8 == 0 and K % 8 == 0


# (C, K, HW) -> (smallest, largest) measured batch N of the --only-tail-gap
# table (bench/bench_mobilenet.py) whose median beat ``pw_conv_fwd`` +
# ``gap_fwd`` by more than that pair's spread in both of two runs (rule and
# figures: docs/KERNELS.md, "pointwise_gap.hip").
_PW_GAP_MEASURED = {
    (320, 1280, 49): (16, 256),        # MobileNetV2 tail @224: 1.71-1.77x, 1.89-1.90x, 1.73-1.74x
}


def pw_gap_route(C: int, K: int, HW: int, N: int) -> bool:
    """True: a frozen 1x1 conv C -> K + BN + activation over ``N`` images of
    ``HW`` pixels whose only reader is the global average pool runs on
    ``k_pw_conv_gap`` (``hip/pointwise_gap.hip``); False: on ``pw_conv_fwd``
    and ``gap_fwd``. ``DDLW_TAIL_GAP``, read per call: ``0`` -> never; ``1``
    -> every supported shape; unset -> the measured winners only, each
    within its measured batch range."""
    if N <= 0 or HW <= 0 or not pw_conv_gap_supported(C, K):
        return False
    return _route_mode("DDLW_TAIL_GAP", _PW_GAP_MEASURED, (C, K, HW), N)


@functools.lru_cache(maxsize=8)
def _cu_count(index: int) -> int:
    return torch.cuda.get_device_properties(index).multi_processor_count


def _pw_gap_imgs(N: int, K: int, device: torch.device) -> int:
    """Images per workgroup: the larger of 4 and 2 that still leaves a
    workgroup for every second CU, else 1. Measured at 7x7, 320 -> 1280
    (docs/KERNELS.md, "pointwise_gap.hip"): 4 is the fastest at batch 64 (160
    workgroups on 256 CUs) and 256, 1 and 2 tie at batch 16, and 8 loses to 4
    everywhere (the weight slab is amortized by then; fewer workgroups only
    lengthen the tail)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    cus, ktiles = _cu_count(index), -(-K // 128)
    for imgs in (4, 2):
        if 2 * -(-N // imgs) * ktiles >= cus:
            return imgs
    return 1


def pw_conv_gap_fwd(x: torch.Tensor, weight: torch.Tensor,
                    scale: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, act: int = 0,
                    out: Optional[torch.Tensor] = None,
                    imgs: Optional[int] = None) -> torch.Tensor:
    """``gap_fwd(pw_conv_fwd(x, weight, scale, bias, act))`` in one launch,
    bit for bit, without the [N,K,H,W] tensor: 1x1 stride-1 conv, folded BN,
    activation (0 none / 1 ReLU / 2 ReLU6), rounding to bf16, then the mean
    over H*W. x channels_last bf16 [N,C,H,W]; weight [K,C,1,1] or [K,C];
    scale/bias fp32 [K], both or neither. Returns (or writes into ``out``)
    bf16 [N,K]. ``imgs``: consecutive images per workgroup; ``None`` takes
    ``_pw_gap_imgs``'s choice."""
    who = "pw_conv_gap_fwd"
    if x.dim() != 4:
        raise ValueError(f"{who}: x must be [N,C,H,W], got {tuple(x.shape)}")
    n, c, h, w_ = x.shape
    if weight.dim() not in (2, 4) or tuple(weight.shape[1:]) not in ((c,), (c, 1, 1)):
        raise ValueError(f"{who}: weight is {tuple(weight.shape)}, x has {c} channels")
    K = weight.shape[0]
    if not pw_conv_gap_supported(c, K):
        raise ValueError(f"{who}: C={c}, K={K} must be multiples of 8 with "
                         f"8 <= C <= {_PW_GAP_MAX_C}")
    if h * w_ < 1:
        raise ValueError(f"{who}: empty feature map {h}x{w_}")
    if (scale is None) != (bias is None):
        raise ValueError(f"{who}: scale and bias come together")
    if scale is not None:
        scale, bias = _f32c(scale, K), _f32c(bias, K)
    if out is not None:
        if (tuple(out.shape) != (n, K) or out.dtype != torch.bfloat16
                or not out.is_contiguous()):
            raise ValueError(f"{who}: out must be contiguous bf16 {(n, K)}")
        p = out
    else:
        p = torch.empty((n, K), dtype=torch.bfloat16, device=x.device)
    if imgs is None:
        imgs = _pw_gap_imgs(n, K, x.device)
    elif imgs < 1:
        raise ValueError(f"{who}: imgs must be at least 1, got {imgs}")
    launch("pw_conv_gap_fwd", _nhwc(x), _pw_w2(weight), p, scale, bias, int(act),
           n, h * w_, c, K, int(imgs))
    return p


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


# (depth, K) -> (mr, smallest measured M, largest measured M): the rows of the
# --only-pw-deep table (bench/bench_mobilenet.py) whose median beat the
# contender they replace by more than its spread in both of two runs.
_PW_DEEP_MEASURED = {
    (576, 160): (2, 784, 3136),      # frozen 2.2x, fwd+stats 1.16x
    (960, 160): (1, 784, 3136),      # frozen 3.0x, fwd+stats 1.7-1.8x, dgrad of 160->960 1.3-2.4x
    (960, 320): (2, 784, 3136),      # frozen 2.7x, fwd+stats 1.7x
    (1280, 320): (2, 3136, 3136),    # dgrad of 320->1280 1.2x (mr = 1 loses: 0.81x)
    # not (576, 96) at 12544 rows: frozen 1.39x and dgrad 1.13x, but fwd+stats
    # 0.96x, and the route does not know the direction
}


def pw_deep_route(depth: int, K: int, M: int) -> Optional[int]:
    """The ``mr`` (16-row fragments per block tile) with which the pointwise
    GEMM of reduction length ``depth`` onto ``K`` output channels over ``M``
    rows runs on the split-reduction kernel (``hip/pointwise_deep.hip``), or
    ``None`` for the plain kernel. ``DDLW_PW_DEEP``, read per call: ``0`` ->
    never; ``1`` -> every shape the kernel takes with ``depth >= 512`` and at
    most 512 partial rows (what ``bn_finalize_parts`` takes without a fold
    launch); unset -> the measured rows only, each from its smallest to its
    largest measured ``M`` (table and rule: docs/KERNELS.md, "Split-reduction
    pointwise conv")."""
    if depth < 512 or M <= 0 or not pw_conv_supported(depth, K):
        return None  # most layers leave here, before the environment is read
    mode = os.environ.get("DDLW_PW_DEEP", "")[:1]
    if mode == "0":
        return None
    row = _PW_DEEP_MEASURED.get((depth, K))
    if mode == "1":
        mr = row[0] if row is not None else 2
        return mr if -(-M // (16 * mr)) <= _FOLD_ABOVE else None
    if row is not None and row[1] <= M <= row[2]:
        return row[0]
    return None


def _pw_deep_mr(mr: Optional[int], depth: int, K: int, M: int) -> int:
    """``mr`` of an explicit call of the split-reduction kernel."""
    if mr is None:
        mr = pw_deep_route(depth, K, M) or 2
    if mr not in (1, 2):
        raise ValueError(f"pw_conv_deep: mr must be 1 or 2, got {mr}")
    return mr


@functools.lru_cache(maxsize=512)
def _pw_deep_nparts(rows: int, mr: int) -> int:
    return int(query("pw_conv_deep_nparts", rows, mr, None))


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
    mr = pw_deep_route(C, K, rows)
    if mr is None:
        launch("pw_conv_fwd", _nhwc(x), w2, y, res, None, None, 0, rows, C, K)
    else:
        launch("pw_conv_deep_fwd", _nhwc(x), w2, y, res, None, None, 0, rows,
               C, K, mr)
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
    ``[nparts, K]`` tensors to write into. A shape ``pw_deep_route`` names
    runs on the split-reduction kernel, with that kernel's ``nparts``."""
    rows, _ = _rows_c(x)
    return _pw_conv_fwd_stats(x, weight, parts,
                              pw_deep_route(weight.shape[1], weight.shape[0], rows),
                              "pw_conv_fwd_stats")


def pw_conv_deep_fwd_stats(x: torch.Tensor, weight: torch.Tensor, parts=None,
                           mr: Optional[int] = None):
    """``pw_conv_fwd_stats`` on the split-reduction kernel whatever the route
    says: same arguments and returns, one partial row per ``16 * mr`` rows.
    ``mr`` as in ``pw_conv_deep_fwd``."""
    rows, _ = _rows_c(x)
    return _pw_conv_fwd_stats(x, weight, parts,
                              _pw_deep_mr(mr, weight.shape[1], weight.shape[0], rows),
                              "pw_conv_deep_fwd_stats")


def _pw_conv_fwd_stats(x, weight, parts, mr, who: str):
    w2 = _pw_w2(weight)
    K, C = w2.shape
    rows, cx = _rows_c(x)
    assert cx == C, f"{who}: x has {cx} channels, weight {C}"
    if not pw_conv_supported(C, K):
        raise ValueError(f"{who}: C={C}, K={K} must be multiples of 8")
    nparts = _pw_conv_nparts(rows, K) if mr is None else _pw_deep_nparts(rows, mr)
    if parts is None:
        both = torch.empty(2, nparts, K, dtype=torch.float32, device=x.device)
        ps, pq = both[0], both[1]
    else:
        ps, pq = parts
        for t in (ps, pq):
            assert (t.dtype == torch.float32 and t.is_contiguous()
                    and tuple(t.shape) == (nparts, K)), f"{who}: parts"
    y = _pw_out(x, rows, K, None, who)
    if mr is None:
        launch("pw_conv_fwd_stats", _nhwc(x), w2, y, ps, pq, rows, C, K)
    else:
        launch("pw_conv_deep_fwd_stats", _nhwc(x), w2, y, ps, pq, rows, C, K, mr)
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


# ---- depthwise conv + BatchNorm, training path ------------------------------ #


def dw_train_route(direction: str, C: int, stride: int, M: int) -> bool:
    """True: this direction (``"fwd"`` = forward + BN statistics, ``"bwd"`` =
    the stride-1 backward after the BN reduce) of a depthwise 3x3 training
    stage with C channels and M = N*Ho*Wo output rows runs on the fused
    kernel; False: on the kernels it replaces. Verdicts of the table in
    docs/KERNELS.md, "Depthwise conv + BN, training path" (MobileNetV2 @224,
    batch 64, two runs)."""
    if direction not in ("fwd", "bwd"):
        raise ValueError(f"dw_train_route: unknown direction {direction!r}")
    if direction == "bwd":
        # every measured stride-1 shape won (1.01x-1.77x, outside the spread)
        return stride == 1  # no fused stride-2 backward
    # The forward is 1.06x-1.38x on medians at every shape, but from 56x56
    # stride 2 down (M <= 50176) both contenders are ~0.04 ms of launch
    # overhead and the replaced pair's spread (0.008-0.012 ms) covers the
    # difference in at least one run of two: not a win by the rule. Below
    # the smallest measured row count nothing is measured and the shape
    # stays on the fused kernel.
    return not (3136 <= M <= 50176)


@functools.lru_cache(maxsize=512)
def _depthwise_fwd_stats_nparts(rows: int, C: int) -> int:
    return int(query("depthwise_fwd_stats_nparts", rows, C, None))


def depthwise_fwd_stats(x: torch.Tensor, weight: torch.Tensor, stride: int,
                        padding: int, parts=None):
    """Training forward of a depthwise 3x3 conv (stride 1 or 2) with the
    BatchNorm statistics of its output from the epilogue: returns ``(y,
    part_sum, part_sumsq, nparts)`` with the partials fp32 ``[nparts, C]``,
    sums over the bf16 ``y``, ``nparts <= 512``, for ``bn_finalize_parts``.
    ``parts``: a pair of contiguous fp32 ``[nparts, C]`` tensors to write
    into."""
    n, c, h, w = x.shape
    assert tuple(weight.shape) == (c, 1, 3, 3), "depthwise_fwd_stats: weight must be [C,1,3,3]"
    if c % 8 != 0:
        raise ValueError(f"depthwise_fwd_stats: C={c} must be a multiple of 8")
    ho = (h + 2 * padding - 3) // stride + 1
    wo = (w + 2 * padding - 3) // stride + 1
    nparts = _depthwise_fwd_stats_nparts(n * ho * wo, c)
    if parts is None:
        both = torch.empty(2, nparts, c, dtype=torch.float32, device=x.device)
        ps, pq = both[0], both[1]
    else:
        ps, pq = parts
        for t in (ps, pq):
            assert (t.dtype == torch.float32 and t.is_contiguous()
                    and tuple(t.shape) == (nparts, c)), "depthwise_fwd_stats: parts"
    y = torch.empty((n, c, ho, wo), dtype=torch.bfloat16, device=x.device,
                    memory_format=torch.channels_last)
    launch("depthwise_fwd_stats", _nhwc(x), _depthwise_w_t(weight), _nhwc(y),
           ps, pq, n, h, w, c, ho, wo, stride, padding)
    return y, ps, pq, nparts


def depthwise_bwd_bn(dout, mask, y, x, weight, mean, rstd, gamma, dbeta,
                     dgamma, relu: bool, need_dx: bool):
    """Backward of a stride-1 pad-1 depthwise 3x3 conv + BatchNorm stage after
    ``bn_bwd_reduce``, in one kernel: ``dz = bn_bwd_dx(dout, mask, y, ...)``
    is recomputed per tile and feeds the conv's input and weight gradients
    without being stored. Returns ``(dx | None, dw)``: dx channels_last bf16
    like ``x`` (``None`` without ``need_dx``), dw fp32 ``[C,1,3,3]``. No
    atomics, bit-reproducible."""
    n, c, h, w = x.shape
    assert tuple(y.shape) == tuple(dout.shape) == (n, c, h, w), \
        "depthwise_bwd_bn: stride 1, pad 1 (the output has the input's shape)"
    assert tuple(weight.shape) == (c, 1, 3, 3), "depthwise_bwd_bn: weight must be [C,1,3,3]"
    if c % 8 != 0:
        raise ValueError(f"depthwise_bwd_bn: C={c} must be a multiple of 8")
    if relu:
        assert mask is not None and mask.dtype == torch.uint8 \
            and mask.numel() == n * h * w * (c // 8), "depthwise_bwd_bn: mask"
    nparts = int(query("depthwise_bwd_bn_nparts", n, h, w, None))
    part = torch.empty(nparts, 9, c, dtype=torch.float32, device=x.device)
    dw = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=x.device)
    dx = (torch.empty((n, c, h, w), dtype=torch.bfloat16, device=x.device,
                      memory_format=torch.channels_last) if need_dx else None)
    launch("depthwise_bwd_bn", _nhwc(dout), mask if relu else None, _nhwc(y),
           _nhwc(x), _depthwise_w_t(weight), _f32c(mean, c), _f32c(rstd, c),
           _f32c(gamma, c), _f32c(dbeta, c), _f32c(dgamma, c), dx, part, dw,
           n, h, w, c, 1 if relu else 0)
    return dx, dw


# ---- conv + frozen BatchNorm, backward on the gated kernels ----------------- #
#
# One definition for all three (hip/pointwise_frozen.hip): with ``out`` the
# bf16 tensor the folded forward kernel wrote,
#   g16 = gate(out) ? bf16(fp32(dout) * scale[k]) : 0,
#   gate = 1 for act 0 (none), 0 < out < 6 for act 2 (ReLU6),
# formed in registers and never stored.


def pw_gated_supported(C: int, K: int) -> bool:
    """Shapes ``pw_dgrad_gated`` / ``pw_wgrad_gated`` take (conv C -> K)."""
    return pw_conv_supported(C, K)


def dw_gated_supported(C: int, kernel: int = 3, stride: int = 1,
                       padding: int = 1) -> bool:
    """Shapes ``depthwise_bwd_gated`` takes: 3x3, pad 1, stride 1 or 2."""
    return C > 0 and C % 8 == 0 and kernel == 3 and padding == 1 and stride in (1, 2)


# (kind, C, K, stride) -> (smallest, largest measured M): the rows of the
# --only-frozen-bn table (bench/bench_mobilenet.py) that beat the path they
# replace by more than its spread in both of two runs (docs/KERNELS.md,
# "Conv + frozen BatchNorm, backward").
_FROZEN_BN_MEASURED = {
    # features[13:] @224, batch 64: every row won in both runs (the stages are
    # launch-bound at these sizes: one or two launches against three to five)
    ("pw_dgrad", 96, 576, 1): (12544, 12544),     # 2.5x, 1.5x
    ("pw_wgrad", 96, 576, 1): (12544, 12544),     # 2.2x, 1.5x
    ("pw_dgrad", 576, 96, 1): (12544, 12544),     # 2.1x, 1.5x
    ("pw_wgrad", 576, 96, 1): (12544, 12544),     # 2.2x, 1.5x
    ("pw_dgrad", 576, 160, 1): (3136, 3136),      # 2.0x, 1.5x
    ("pw_wgrad", 576, 160, 1): (3136, 3136),      # 2.2x, 1.5x
    ("pw_dgrad", 160, 960, 1): (3136, 3136),      # 1.6x, 1.5x
    ("pw_wgrad", 160, 960, 1): (3136, 3136),      # 2.2x, 1.5x
    ("pw_dgrad", 960, 160, 1): (3136, 3136),      # 2.1x, 1.4x
    ("pw_wgrad", 960, 160, 1): (3136, 3136),      # 2.1x, 1.5x
    ("pw_dgrad", 960, 320, 1): (3136, 3136),      # 2.0x, 1.5x
    ("pw_wgrad", 960, 320, 1): (3136, 3136),      # 2.1x, 1.5x
    ("pw_dgrad", 320, 1280, 1): (3136, 3136),     # 1.1x, 1.4x: the 1280-deep reduction
    ("pw_wgrad", 320, 1280, 1): (3136, 3136),     # 2.1x, 1.5x
    ("dw_bwd", 576, 576, 1): (12544, 12544),      # 1.4x, 1.5x
    ("dw_bwd", 576, 576, 2): (3136, 3136),        # 1.6x, 1.5x
    ("dw_bwd", 960, 960, 1): (3136, 3136),        # 1.9x, 1.5x
}

_FROZEN_BN_KINDS = ("pw_dgrad", "pw_wgrad", "dw_bwd")


def frozen_bn_route(kind: str, C: int, K: int, stride: int, M: int) -> bool:
    """True: this direction of a conv + frozen-BN stage (``"pw_dgrad"`` /
    ``"pw_wgrad"`` of a 1x1 conv C -> K, ``"dw_bwd"`` of a depthwise 3x3 with
    C == K channels) over M output rows runs on the gated kernel; False: on
    the kernels it replaces (g16 formed elementwise, then the plain dgrad /
    wgrad). ``DDLW_FROZEN_BN``, read per call: ``0`` -> never, ``1`` -> every
    supported shape, unset -> the measured winners only."""
    if kind not in _FROZEN_BN_KINDS:
        raise ValueError(f"frozen_bn_route: unknown kind {kind!r}")
    if kind == "dw_bwd":
        if C != K or not dw_gated_supported(C, 3, stride, 1):
            return False
    elif stride != 1 or not pw_gated_supported(C, K):
        return False
    return M > 0 and _route_mode("DDLW_FROZEN_BN", _FROZEN_BN_MEASURED,
                                 (kind, C, K, stride), M)


def _gated_args(who, dout, out, scale, act, K):
    if act not in (0, 2):
        raise ValueError(f"{who}: act must be 0 (none) or 2 (ReLU6), got {act}")
    assert out.shape == dout.shape, f"{who}: out and dout differ in shape"
    return _nhwc(dout), (_nhwc(out) if act == 2 else None), _f32c(scale, K)


def pw_dgrad_gated(dout: torch.Tensor, out: torch.Tensor, weight: torch.Tensor,
                   scale: torch.Tensor, act: int, in_shape,
                   acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of a 1x1 conv + frozen-BN stage: ``dx[m][c] =
    bf16(sum_k g16[m][k] * w[k][c] (+ acc[m][c]))``. dout/out channels_last
    bf16 [N,K,H,W] (or rows [M,K]); weight [K,C,1,1]; scale fp32 [K]; ``acc``
    a dx-shaped bf16 tensor added before the one rounding (the gradient that
    joins at the stage's input). The weight is transposed here per call, as
    ``pw_conv_dgrad`` does (it changes every step)."""
    w2 = _pw_w2(weight)
    K, C = w2.shape
    if not pw_gated_supported(C, K):
        raise ValueError(f"pw_dgrad_gated: C={C}, K={K} must be multiples of 8")
    rows, kd = _rows_c(dout)
    assert kd == K, f"pw_dgrad_gated: dout has {kd} channels, weight {K}"
    dout, out, scale = _gated_args("pw_dgrad_gated", dout, out, scale, act, K)
    dx = _pw_out(dout, rows, C, None, "pw_dgrad_gated")
    assert tuple(dx.shape) == tuple(in_shape), "pw_dgrad_gated: in_shape"
    if acc is not None:
        assert acc.shape == dx.shape, "pw_dgrad_gated: acc must match dx"
        acc = _nhwc(acc)
    launch("pw_dgrad_gated", dout, out, w2.t().contiguous(), scale, dx, acc,
           int(act), rows, C, K)
    return dx


def pw_wgrad_gated(dout: torch.Tensor, out: torch.Tensor, x: torch.Tensor,
                   scale: torch.Tensor, act: int, weight_shape) -> torch.Tensor:
    """Weight gradient of a 1x1 conv + frozen-BN stage, bf16 of
    ``weight_shape``: ``dw[k][c] = bf16(sum_m g16[m][k] * x[m][c])``. Row
    slices into fp32 partials, then a fixed-order fold: bit-reproducible."""
    K, C = int(weight_shape[0]), int(weight_shape[1])
    if not pw_gated_supported(C, K):
        raise ValueError(f"pw_wgrad_gated: C={C}, K={K} must be multiples of 8")
    rows, kd = _rows_c(dout)
    rx, cx = _rows_c(x)
    assert (kd, cx, rx) == (K, C, rows), "pw_wgrad_gated: dout / x / weight_shape disagree"
    dout, out, scale = _gated_args("pw_wgrad_gated", dout, out, scale, act, K)
    dw = torch.empty(tuple(weight_shape), dtype=torch.bfloat16, device=x.device)
    if rows == 0:
        return dw.zero_()
    nparts = int(query("pw_wgrad_gated_nparts", rows, C, K, None))
    part = torch.empty(nparts, K, C, dtype=torch.float32, device=x.device)
    launch("pw_wgrad_gated", dout, out, _nhwc(x), scale, part, dw, int(act),
           rows, C, K)
    return dw


def depthwise_bwd_gated(dout: torch.Tensor, out: torch.Tensor, x: torch.Tensor,
                        weight: torch.Tensor, scale: torch.Tensor, act: int,
                        stride: int, need_dx: bool):
    """Backward of a depthwise 3x3 pad-1 conv (stride 1 or 2) + frozen-BN
    stage in one kernel: returns ``(dx | None, dw)``, dx channels_last bf16
    like ``x`` (the transposed conv of g16 with the weight), dw fp32
    ``[C,1,3,3]`` like ``depthwise_wgrad``. Bit-reproducible."""
    n, c, h, w = x.shape
    assert tuple(weight.shape) == (c, 1, 3, 3), "depthwise_bwd_gated: weight must be [C,1,3,3]"
    if not dw_gated_supported(c, 3, stride, 1):
        raise ValueError(f"depthwise_bwd_gated: C={c}, stride={stride} not supported")
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    assert tuple(dout.shape) == (n, c, ho, wo), \
        f"depthwise_bwd_gated: dout is {tuple(dout.shape)}, the output is {(n, c, ho, wo)}"
    dout, out, scale = _gated_args("depthwise_bwd_gated", dout, out, scale, act, c)
    nparts = int(query("depthwise_bwd_bn_nparts", n, h, w, None))
    part = torch.empty(nparts, 9, c, dtype=torch.float32, device=x.device)
    dw = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=x.device)
    dx = (torch.empty((n, c, h, w), dtype=torch.bfloat16, device=x.device,
                      memory_format=torch.channels_last) if need_dx else None)
    launch("depthwise_bwd_gated", dout, out, _nhwc(x),
           _depthwise_w_t(weight) if need_dx else None, scale, dx, part, dw,
           n, h, w, c, ho, wo, stride, int(act))
    return dx, dw


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


# ---- classifier head: dropout + dense in one launch each way ---------------- #

_HEAD_DENSE_MAX_K = 64


def head_dense_supported(C: int, K: int) -> bool:
    """Shapes the ``head_dense`` kernels take: 16-byte bf16x8 vectors along
    the features and at most four 16-class MFMA fragments."""
    return C >= 8 and C % 8 == 0 and 1 <= K <= _HEAD_DENSE_MAX_K


# (C, K) -> (smallest, largest) measured batch N of the --only-head-dense
# table (bench/bench_mobilenet.py) at which the fused stage beat dropout +
# nn.Linear by more than that stage's spread in both of two runs (rule and
# figures: docs/KERNELS.md, "head_dense.hip").
_HEAD_DENSE_MEASURED = {
    # MobileNetV2 head: fwd 2.1x, fwd+bwd 1.05-1.47x, with dx 1.47-1.80x. At
    # batch 256 the with-dx row was inside a 0.09 ms spread in one run: off.
    (1280, 5): (16, 64),
}


def head_dense_route(C: int, K: int, N: int) -> bool:
    """True: dropout + dense C -> K over ``N`` rows of pooled features runs
    on the ``head_dense`` kernels (``hip/head_dense.hip``); False: on
    ``dropout_fwd`` and ``nn.Linear``. ``DDLW_HEAD_DENSE``, read per call:
    ``0`` -> never; ``1`` -> every supported shape; unset -> the measured
    winners only, each within its measured batch range."""
    if N < 1 or not head_dense_supported(C, K):
        return False
    return _route_mode("DDLW_HEAD_DENSE", _HEAD_DENSE_MEASURED, (C, K), N)


def _head_dense_args(who, x, w, p):
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise ValueError(f"{who}: x is {tuple(x.shape)}, w is {tuple(w.shape)}; "
                         f"want [N,C] and [K,C]")
    (n, c), k = x.shape, w.shape[0]
    if n < 1 or not head_dense_supported(c, k):
        raise ValueError(f"{who}: N={n}, C={c}, K={k}: need N >= 1, C a multiple "
                         f"of 8 and 1 <= K <= {_HEAD_DENSE_MAX_K}")
    for name, t in (("x", x), ("w", w)):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous bf16, got {t.dtype}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{who}: p must be in [0, 1), got {p}")
    return n, c, k


def head_dense_fwd(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor],
                   p: float, seed: int) -> torch.Tensor:
    """``dropout_fwd(x, p, seed)[0] @ w.T + b`` in one launch, without the
    dropped activations or a mask: x bf16 [N,C], w bf16 [K,C], b bf16 [K] or
    None; fp32 accumulation, one rounding. ``p == 0`` is the plain dense
    layer. Returns bf16 [N,K]."""
    who = "head_dense_fwd"
    n, c, k = _head_dense_args(who, x, w, p)
    if b is not None and (b.dtype != torch.bfloat16 or tuple(b.shape) != (k,)
                          or not b.is_contiguous()):
        raise ValueError(f"{who}: b must be contiguous bf16 [{k}]")
    y = torch.empty((n, k), dtype=torch.bfloat16, device=x.device)
    launch("head_dense_fwd", x, w, b, y, n, c, k, float(p), seed & (2**64 - 1))
    return y


def head_dense_bwd(dlogits: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                   p: float, seed: int, want_dx: bool, want_db: bool):
    """Backward of ``head_dense_fwd`` from ``dlogits`` [N,K] (bf16, or fp32
    rounded to bf16 once as it is loaded) and the forward's ``(x, w, p,
    seed)``: returns ``(dW [K,C], db [K] or None, dx [N,C] or None)``, bf16.
    The dropped activations are regenerated, not read."""
    who = "head_dense_bwd"
    n, c, k = _head_dense_args(who, x, w, p)
    if (tuple(dlogits.shape) != (n, k) or not dlogits.is_contiguous()
            or dlogits.dtype not in (torch.bfloat16, torch.float32)):
        raise ValueError(f"{who}: dlogits must be contiguous bf16 or fp32 {(n, k)}, "
                         f"got {dlogits.dtype} {tuple(dlogits.shape)}")
    dw = torch.empty_like(w)
    db = torch.empty(k, dtype=torch.bfloat16, device=x.device) if want_db else None
    dx = torch.empty_like(x) if want_dx else None
    launch("head_dense_bwd", dlogits, x, w, dw, db, dx, n, c, k, float(p),
           seed & (2**64 - 1), 1 if dlogits.dtype == torch.float32 else 0)
    return dw, db, dx


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
