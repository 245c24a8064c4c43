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
from ..ops.layers import BatchNormAct2d, GlobalAvgPool2d
from ..ops import mbconv


def _pointwise(in_ch: int, out_ch: int) -> Conv2d:
    """A 1x1 conv opted in to the pointwise training kernels (an instance
    attribute: no new parameter, buffer or state_dict key)."""
    conv = Conv2d(in_ch, out_ch, 1, bias=False)
    conv.pw_train = True
    return conv


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

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x, start = self.stem_entry(x)
        n = len(self.features)
        tail_conv, tail_bn = self.features[n - 3], self.features[n - 2]
        if (mbconv.eval_fold_enabled(self, x)
                and tail_bn.running_mean.dtype == torch.float32):
            # frozen forward: the blocks fuse themselves; the 320->1280 tail
            # conv + BN + ReLU6 is one pointwise kernel as well
            for m in self.features[start: n - 3]:
                x = m(x)
            return mbconv.conv_bn_eval(
                tail_conv, tail_bn,
                x.contiguous(memory_format=torch.channels_last))
        if start == 0:
            return self.features(x)
        for m in self.features[start:]:
            x = m(x)
        return x


class FrozenBase(nn.Module):
    """Wraps a base so it stays in eval mode (frozen BN -> moving stats,
    reference ``.../02_model_training_single_node.py:167-169``).

    ``fine_tune_at=k`` unfreezes ``base.features[k:]``: those children get
    ``requires_grad=True`` and follow ``train()``/``eval()``;
    ``base.features[:k]`` keeps ``requires_grad=False``, stays in ``eval()``
    and runs under ``no_grad``. ``None`` (default) or ``len(features)``
    freezes everything, with the whole base in one ``no_grad`` forward.
    """

    accepts_uint8 = True  # hands a uint8 batch to ``base.stem_entry``

    def __init__(self, base: nn.Module, fine_tune_at: Optional[int] = None):
        super().__init__()
        self.base = base
        self.set_fine_tune_at(fine_tune_at)

    def _num_features(self) -> Optional[int]:
        feats = getattr(self.base, "features", None)
        return len(feats) if isinstance(feats, nn.Sequential) else None

    def set_fine_tune_at(self, fine_tune_at: Optional[int]) -> None:
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
        self.train(self.training)

    @property
    def fine_tune_at(self) -> Optional[int]:
        return self._split

    def _fully_frozen(self) -> bool:
        return self._split is None or self._split == self._num_features()

    def train(self, mode: bool = True) -> "FrozenBase":
        super().train(mode)
        if self._fully_frozen():
            # stay frozen: never switch the base to train-mode BN
            self.base.eval()
        else:
            for m in self.base.features[: self._split]:
                m.eval()
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fully_frozen():
            with torch.no_grad():
                return self.base(x)
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
        for m in feats[max(start, self._split):]:
            x = m(x)
        return x


class TransferModel(nn.Module):
    """Frozen base -> GAP -> Dropout -> Dense(num_classes) logits
    (reference ``.../02_model_training_single_node.py:171-176``).
    ``fine_tune_at``: see ``FrozenBase``."""

    accepts_uint8 = True  # the base takes the uint8 batch

    def __init__(self, channels: int = 3, num_classes: int = 5, dropout: float = 0.5,
                 fine_tune_at: Optional[int] = None):
        super().__init__()
        self.base = FrozenBase(MobileNetV2(channels), fine_tune_at)
        self.global_average_pooling = GlobalAvgPool2d()
        from ..ops.layers import Dropout as DdlwDropout

        self.dropout = DdlwDropout(dropout)  # K7 kernel on GPU, stock on CPU
        self.classifier = nn.Linear(1280, num_classes)

    def set_fine_tune_at(self, fine_tune_at: Optional[int]) -> None:
        """Switch the frozen/trainable split of the base in place (phase 2
        after head training); a saved model keeps the new split. An
        optimizer built earlier does not see newly trainable parameters."""
        self.base.set_fine_tune_at(fine_tune_at)
        spec = getattr(self, "_ddlw_builder_spec", None)
        if spec is not None:
            spec[1]["fine_tune_at"] = fine_tune_at

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.base(x)
        x = self.global_average_pooling(x)  # fused GAP -> (N, C)
        x = self.dropout(x)
        return self.classifier(x.to(self.classifier.weight.dtype))


def build_model(
    img_height: int = 224,
    img_width: int = 224,
    img_channels: int = 3,
    num_classes: int = 5,
    dropout: float = 0.5,
    fine_tune_at: Optional[int] = None,
) -> TransferModel:
    """``fine_tune_at=k`` makes ``features[k:]`` of the MobileNetV2 base
    trainable (23 children: 0-2 stem, 3-19 inverted residuals, 20-22 the
    1x1 tail); ``None`` or 23 keeps the whole base frozen. The trainable
    part follows the reference's per-layer ``trainable`` flags: its
    BatchNorms use batch statistics in training (not Keras's
    ``training=False`` fine-tuning recipe)."""
    m = TransferModel(channels=img_channels, num_classes=num_classes, dropout=dropout,
                      fine_tune_at=fine_tune_at)
    return tag_model(
        m,
        "mobilenet_v2_head",
        dict(
            img_height=img_height,
            img_width=img_width,
            img_channels=img_channels,
            num_classes=num_classes,
            dropout=dropout,
            fine_tune_at=fine_tune_at,
        ),
    )
