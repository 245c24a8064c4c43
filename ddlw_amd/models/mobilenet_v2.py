"""MobileNetV2 + transfer-learning head — the reference's ``build_model()``.

Reference contract (``Part 1 .../02_model_training_single_node.py:159-178``):
``build_model(img_height, img_width, img_channels, num_classes, dropout)`` ->
frozen MobileNetV2 base (include_top=False) -> GlobalAveragePooling ->
Dropout -> Dense(num_classes) producing *logits*.

Faithfulness notes: the base is frozen layer by
layer, so its BatchNorms must run with *moving statistics* even in training
mode — here the base is put in eval() and its params have
``requires_grad=False``; ``FrozenBase.train()`` keeps it in eval mode.

Fine-tuning (``fine_tune_at=k``): ``features[k:]`` becomes trainable while
``features[:k]`` stays frozen as above — the second phase of transfer
learning (train the head, then unfreeze the top of the base at a low
learning rate). The trainable suffix follows ``train()``/``eval()`` like any
module, so its BatchNorms use *batch* statistics in training. That is what
the reference's per-layer ``trainable`` flags give; it is NOT the Keras
fine-tuning recipe that keeps calling the base with ``training=False``.
``fine_tune_bn="frozen"`` selects that recipe, with frozen BatchNorms
(``FrozenBase``).

Activations: every BN + ReLU6 pair is one fused ``BatchNormAct2d(act=
"relu6")``; an ``nn.Identity`` keeps the old ReLU6 slot so ``state_dict``
keys and ``features`` indices are unchanged and saved models still load.

Input: a float batch, or the ``torch.uint8`` N x C x H x W batch over NHWC
memory (``u8_nhwc.permute(0, 3, 1, 2)``) that the decode pool and the H2D ring
deliver — ``preprocess_input`` (``x / 127.5 - 1``) then belongs to the model,
and on the frozen bf16 route it is fused with the stem conv, its BN and ReLU6
into one kernel (``MobileNetV2.stem_entry``, ``ops/mbconv.py``). A training
stem marked by ``enable_u8_train_stem`` (the bf16 policy does) can run from the
bytes as well: ``DDLW_STEM_U8_TRAIN=1``, off by default (docs/KERNELS.md).

No pretrained weights exist in this offline environment, so the base is
randomly initialised (documented deviation; the benchmark configs use
random-init weights anyway, BASELINE.json).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ..core.model_io import tag_model
from ..ops.conv import Conv2d
from ..ops.layers import (BatchNormAct2d, GlobalAvgPool2d, dropout_linear,
                          dropout_linear_route)
from ..ops import mbconv


def _pointwise(in_ch: int, out_ch: int) -> Conv2d:
    """A 1x1 conv opted in to the pointwise training kernels (an instance
    attribute: no new parameter, buffer or state_dict key)."""
    conv = Conv2d(in_ch, out_ch, 1, bias=False)
    conv.pw_train = True
    return conv


_POOL = GlobalAvgPool2d()  # stateless: the pool of ``forward(x, pooled=True)``


class InvertedResidual(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, stride: int, expand: int):
        super().__init__()
        hidden = in_ch * expand
        self.use_res = stride == 1 and in_ch == out_ch
        layers = []
        if expand != 1:
            layers += [
                _pointwise(in_ch, hidden),
                BatchNormAct2d(hidden, act="relu6"),
                nn.Identity(),  # old ReLU6 slot (fused into the BN above)
            ]
        layers += [
            Conv2d(hidden, hidden, 3, stride=stride, padding=1, groups=hidden, bias=False),
            BatchNormAct2d(hidden, act="relu6"),
            nn.Identity(),
            _pointwise(hidden, out_ch),
            BatchNormAct2d(out_ch),
        ]
        self.conv = nn.Sequential(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if mbconv.inverted_residual_eval_fusable(self, x):
            # frozen block: BN folded into the conv epilogues (ops/mbconv.py)
            return mbconv.inverted_residual_eval_forward(self, x)
        if mbconv.inverted_residual_train_fusable(self, x):
            # trainable block: pointwise conv + BN stages with the statistics
            # out of the conv epilogue (ops/mbconv.py)
            return mbconv.inverted_residual_train_forward(self, x)
        if mbconv.inverted_residual_frozen_bn_fusable(self, x):
            # trainable convs under frozen BNs (``fine_tune_bn="frozen"``):
            # folded forward kernels, gated backward kernels (ops/mbconv.py)
            return mbconv.inverted_residual_frozen_bn_forward(self, x)
        return x + self.conv(x) if self.use_res else self.conv(x)


# (expand t, out channels c, repeats n, first stride s) — standard MobileNetV2
_V2_CFG = [
    (1, 16, 1, 1),
    (6, 24, 2, 2),
    (6, 32, 3, 2),
    (6, 64, 4, 2),
    (6, 96, 3, 1),
    (6, 160, 3, 2),
    (6, 320, 1, 1),
]


class MobileNetV2(nn.Module):
    """Feature extractor (include_top=False): output B x 1280 x H/32 x W/32."""

    accepts_uint8 = True  # ``stem_entry`` normalizes; read by ops.prepare_batch

    def __init__(self, channels: int = 3):
        super().__init__()
        blocks = [
            Conv2d(channels, 32, 3, stride=2, padding=1, bias=False),
            BatchNormAct2d(32, act="relu6"),
            nn.Identity(),
        ]
        in_ch = 32
        for t, c, n, s in _V2_CFG:
            for i in range(n):
                blocks.append(InvertedResidual(in_ch, c, s if i == 0 else 1, t))
                in_ch = c
        blocks += [
            _pointwise(in_ch, 1280),
            BatchNormAct2d(1280, act="relu6"),
            nn.Identity(),
        ]
        self.features = nn.Sequential(*blocks)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, Conv2d)):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, (nn.BatchNorm2d, BatchNormAct2d)):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def enable_u8_train_stem(self, flag: bool = True) -> None:
        """Opt the stem in to (or out of) the training-mode uint8 kernels:
        the mark ``u8_train`` on ``features[0]``, an instance attribute like
        ``Conv2d.pw_train`` (no parameter, buffer or state_dict key, kept by
        ``deepcopy``, not saved). ``ops.precision.apply_bf16_policy`` sets it;
        an unmarked net routes exactly as before."""
        self.features[0].u8_train = bool(flag)

    def stem_entry(self, x: torch.Tensor, frozen_stem: bool = True):
        """The one entry for a batch, used by ``forward`` and by
        ``FrozenBase``'s split forward: returns ``(h, start)`` and the caller
        continues at ``features[start]``. A float batch is returned as it is
        with ``start = 0``. A ``torch.uint8`` batch (N x C x H x W, channels_last:
        ``u8_nhwc.permute(0, 3, 1, 2)``) is what the decode pool delivers and
        ``preprocess_input`` belongs to the model: when the stem is frozen
        (``frozen_stem``) and ``mbconv.stem_u8_fusable`` holds, normalize +
        stem conv + BN + ReLU6 run as one kernel and ``start = 3``; otherwise
        the batch is normalized once and ``start = 0``.

        A stem marked by ``enable_u8_train_stem`` adds two routes, both
        decided by the caller's grad mode: a TRAINING stem
        (``mbconv.stem_u8_train_fusable``) runs on the stage Function of the
        uint8 stem kernels, ``start = 3``, and the normalized batch is never
        written; and a trainable stem that is merely evaluated (eval mode
        under no-grad: validation during ``fit``) takes the fused frozen
        kernel like a frozen one, since its BN uses the running statistics."""
        if x.dtype != torch.uint8:
            return x, 0
        if mbconv.stem_u8_train_fusable(self, x):
            return mbconv.stem_u8_train_forward(self, x), 3
        # a trainable stem evaluated under no-grad: the fused kernel, on the
        # live weight and BN tensors (nothing cached: they are being trained)
        live = (not frozen_stem and getattr(self.features[0], "u8_train", False)
                and not torch.is_grad_enabled())
        if (frozen_stem or live) and mbconv.stem_u8_fusable(self, x):
            return mbconv.stem_u8_forward(self, x, fresh=live), 3
        with torch.no_grad():
            return mbconv.normalize_u8_input(x, self.features[0].weight), 0

    def forward(self, x: torch.Tensor, pooled: bool = False) -> torch.Tensor:
        """``pooled=True`` returns the N x 1280 global-average-pooled features
        (``GlobalAvgPool2d`` of the plain result) on every branch; on the
        frozen-fold branch the tail conv and the pool may then be one kernel
        (``mbconv.conv_bn_gap_eval``)."""
        x, start = self.stem_entry(x)
        n = len(self.features)
        tail_conv, tail_bn = self.features[n - 3], self.features[n - 2]
        if (mbconv.eval_fold_enabled(self, x)
                and tail_bn.running_mean.dtype == torch.float32):
            # frozen forward: the blocks fuse themselves; the 320->1280 tail
            # conv + BN + ReLU6 is one pointwise kernel as well
            for m in self.features[start: n - 3]:
                x = m(x)
            x = x.contiguous(memory_format=torch.channels_last)
            if pooled:
                return mbconv.conv_bn_gap_eval(tail_conv, tail_bn, x)
            return mbconv.conv_bn_eval(tail_conv, tail_bn, x)
        if start == 0:
            x = self.features(x)
        else:
            for m in self.features[start:]:
                x = m(x)
        return _POOL(x) if pooled else x


class FrozenBase(nn.Module):
    """Wraps a base so it stays in eval mode (frozen BN -> moving stats,
    reference ``.../02_model_training_single_node.py:167-169``).

    ``fine_tune_at=k`` unfreezes ``base.features[k:]``: those children get
    ``requires_grad=True`` and follow ``train()``/``eval()``;
    ``base.features[:k]`` keeps ``requires_grad=False``, stays in ``eval()``
    and runs under ``no_grad``. ``None`` (default) or ``len(features)``
    freezes everything, with the whole base in one ``no_grad`` forward.

    ``fine_tune_bn`` says what the BatchNorms of the trainable suffix do.
    ``"batch"`` (default): they train on batch statistics, as above.
    ``"frozen"``: the Keras fine-tuning recipe's ``training=False`` base in
    the ``FrozenBatchNorm2d`` convention. Every BN of the base stays in eval
    mode, its ``weight`` / ``bias`` get ``requires_grad=False``, its running
    buffers and ``num_batches_tracked`` are never touched, and only the conv
    weights of the suffix train. (Keras would still train gamma / beta under
    the moving statistics; here each BN is a constant per-channel affine.)
    On CUDA bf16 such a block runs on the folded forward kernels and the
    gated backward kernels (``ops/mbconv.py``, ``DDLW_FROZEN_BN``).
    """

    accepts_uint8 = True  # hands a uint8 batch to ``base.stem_entry``
    FINE_TUNE_BN = ("batch", "frozen")

    def __init__(self, base: nn.Module, fine_tune_at: Optional[int] = None,
                 fine_tune_bn: str = "batch"):
        super().__init__()
        self.base = base
        self._bn_mode = "batch"
        self.set_fine_tune_at(fine_tune_at, fine_tune_bn)

    def _num_features(self) -> Optional[int]:
        feats = getattr(self.base, "features", None)
        return len(feats) if isinstance(feats, nn.Sequential) else None

    @property
    def fine_tune_bn(self) -> str:
        return self._bn_mode

    def set_fine_tune_at(self, fine_tune_at: Optional[int],
                         fine_tune_bn: Optional[str] = None) -> None:
        """``fine_tune_bn=None`` keeps the current BN mode."""
        if fine_tune_bn is not None:
            if fine_tune_bn not in self.FINE_TUNE_BN:
                raise ValueError(f"fine_tune_bn must be one of {self.FINE_TUNE_BN}, "
                                 f"got {fine_tune_bn!r}")
            self._bn_mode = fine_tune_bn
        n = self._num_features()
        if fine_tune_at is None:
            k = n
        else:
            if n is None:
                raise ValueError("fine_tune_at needs a base with a `features` Sequential")
            if (isinstance(fine_tune_at, bool) or not isinstance(fine_tune_at, int)
                    or not 0 <= fine_tune_at <= n):
                raise ValueError(
                    f"fine_tune_at must be None or an int in [0, {n}], got {fine_tune_at!r}"
                )
            k = fine_tune_at
        self._split = k  # == n (or None without `features`): fully frozen
        if k is None or k == n:
            for p in self.base.parameters():
                p.requires_grad = False
        else:
            for i, m in enumerate(self.base.features):
                for p in m.parameters():
                    p.requires_grad = i >= k
            if self._bn_mode == "frozen":
                for m in self.base.modules():
                    if isinstance(m, (nn.BatchNorm2d, BatchNormAct2d)):
                        m.weight.requires_grad = False
                        m.bias.requires_grad = False
        self.train(self.training)

    @property
    def fine_tune_at(self) -> Optional[int]:
        return self._split

    def _fully_frozen(self) -> bool:
        return self._split is None or self._split == self._num_features()

    def train(self, mode: bool = True) -> "FrozenBase":
        super().train(mode)
        if self._fully_frozen() or self._bn_mode == "frozen":
            # stay frozen: never switch the base to train-mode BN (nothing
            # else in the base depends on the mode)
            self.base.eval()
        else:
            for m in self.base.features[: self._split]:
                m.eval()
        return self

    def forward(self, x: torch.Tensor, pooled: bool = False) -> torch.Tensor:
        """``pooled=True`` (a ``MobileNetV2`` base): the global-average-pooled
        features. Fully frozen, the base pools itself (``MobileNetV2.forward``);
        with a trainable suffix the module path pools, so autograd sees what
        it saw."""
        if self._fully_frozen():
            with torch.no_grad():
                return self.base(x, pooled=True) if pooled else self.base(x)
        feats = self.base.features
        start = 0
        if x.dtype == torch.uint8:
            if self._split >= 3:
                # frozen stem: the fused kernel
                with torch.no_grad():
                    x, start = self.base.stem_entry(x, frozen_stem=True)
            else:
                # a trainable stem gets the normalized batch and its modules,
                # or, marked, the uint8 stem kernels as the caller's grad
                # mode says (``stem_entry``); it normalizes under no_grad
                x, start = self.base.stem_entry(x, frozen_stem=False)
        with torch.no_grad():
            for m in feats[start: self._split]:
                x = m(x)
        first, n = max(start, self._split), len(feats)
        if (self._bn_mode == "frozen" and isinstance(self.base, MobileNetV2)
                and first <= n - 3):
            # the 320 -> 1280 tail conv + BN + ReLU6 of a frozen-BN suffix is
            # one pointwise stage (the blocks route themselves)
            for m in feats[first: n - 3]:
                x = m(x)
            if mbconv.conv_bn_frozen_fusable(feats[n - 3], feats[n - 2], x):
                x = mbconv.conv_bn_frozen(feats[n - 3], feats[n - 2], x)
                return _POOL(x) if pooled else x
            first = n - 3
        for m in feats[first:]:
            x = m(x)
        return _POOL(x) if pooled else x


class TransferModel(nn.Module):
    """Frozen base -> GAP -> Dropout -> Dense(num_classes) logits
    (reference ``.../02_model_training_single_node.py:171-176``).
    ``fine_tune_at``, ``fine_tune_bn``: see ``FrozenBase``."""

    accepts_uint8 = True  # the base takes the uint8 batch

    def __init__(self, channels: int = 3, num_classes: int = 5, dropout: float = 0.5,
                 fine_tune_at: Optional[int] = None, fine_tune_bn: str = "batch"):
        super().__init__()
        self.base = FrozenBase(MobileNetV2(channels), fine_tune_at, fine_tune_bn)
        self.global_average_pooling = GlobalAvgPool2d()
        from ..ops.layers import Dropout as DdlwDropout

        self.dropout = DdlwDropout(dropout)  # K7 kernel on GPU, stock on CPU
        self.classifier = nn.Linear(1280, num_classes)

    def set_fine_tune_at(self, fine_tune_at: Optional[int],
                         fine_tune_bn: Optional[str] = None) -> None:
        """Switch the frozen/trainable split of the base in place (phase 2
        after head training), and with ``fine_tune_bn`` the BN mode of the
        suffix (``None`` keeps it); a saved model keeps both. An optimizer
        built earlier does not see newly trainable parameters."""
        self.base.set_fine_tune_at(fine_tune_at, fine_tune_bn)
        spec = getattr(self, "_ddlw_builder_spec", None)
        if spec is not None:
            spec[1]["fine_tune_at"] = fine_tune_at
            # the key exists only for "frozen": a default spec stays as it was
            spec[1].pop("fine_tune_bn", None)
            if self.base.fine_tune_bn == "frozen":
                spec[1]["fine_tune_bn"] = "frozen"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if (type(self.global_average_pooling) is GlobalAvgPool2d
                and isinstance(self.base.base, MobileNetV2)):
            # the stock pool: the base pools, and a frozen one may fuse its
            # tail conv with the pool (ops/mbconv.py, ``conv_bn_gap_eval``)
            x = self.base(x, pooled=True)
            if dropout_linear_route(x, self.dropout, self.classifier):
                # dropout + dense in one kernel each way (hip/head_dense.hip)
                return dropout_linear(x, self.dropout, self.classifier)
        else:
            x = self.global_average_pooling(self.base(x))  # fused GAP -> (N, C)
        x = self.dropout(x)
        return self.classifier(x.to(self.classifier.weight.dtype))


def build_model(
    img_height: int = 224,
    img_width: int = 224,
    img_channels: int = 3,
    num_classes: int = 5,
    dropout: float = 0.5,
    fine_tune_at: Optional[int] = None,
    fine_tune_bn: str = "batch",
) -> TransferModel:
    """``fine_tune_at=k`` makes ``features[k:]`` of the MobileNetV2 base
    trainable (23 children: 0-2 stem, 3-19 inverted residuals, 20-22 the
    1x1 tail); ``None`` or 23 keeps the whole base frozen. With
    ``fine_tune_bn="batch"`` (default) the trainable part follows the
    reference's per-layer ``trainable`` flags: its BatchNorms use batch
    statistics in training. ``fine_tune_bn="frozen"`` is the Keras
    ``training=False`` fine-tuning recipe with frozen BatchNorms: moving
    statistics, constant gamma / beta, only the conv weights of the suffix
    train (``FrozenBase``)."""
    m = TransferModel(channels=img_channels, num_classes=num_classes, dropout=dropout,
                      fine_tune_at=fine_tune_at, fine_tune_bn=fine_tune_bn)
    spec = dict(
        img_height=img_height,
        img_width=img_width,
        img_channels=img_channels,
        num_classes=num_classes,
        dropout=dropout,
        fine_tune_at=fine_tune_at,
    )
    if fine_tune_bn == "frozen":  # only then: a default spec stays as it was
        spec["fine_tune_bn"] = "frozen"
    return tag_model(m, "mobilenet_v2_head", spec)
