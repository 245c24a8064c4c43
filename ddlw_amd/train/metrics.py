"""Loss and accuracy summed on the model's device.

The per-step path of ``Model.fit`` reads both back with ``float()`` after
every step, two host syncs. ``DeviceMetrics`` keeps the running sums in an
fp64 [4] tensor that the loss kernel updates itself
(``ops.softmax_ce_metrics``), and reads it once per epoch
(``fit(..., metrics_on_device=True)``).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch


class DeviceMetrics:
    """Running sums of the per-step mean loss and accuracy on ``device``.

    ``accum`` is fp64 [4]: (sum of step losses, sum of step accuracies,
    steps, labels outside the class range). Each step adds its fp32 values
    widened to double, which is what ``agg[k] += float(v)`` computes on the
    host, so an epoch's figures are the per-step path's figures.
    ``step_out`` is the last update's fp32 [2] (loss, accuracy), on the
    device; nothing here reads it."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.accum = torch.zeros(4, dtype=torch.float64, device=self.device)
        self.step_out: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.accum.zero_()

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """Add one step; returns its differentiable fp32 0-dim mean loss."""
        from ..ops.layers import softmax_ce_metrics

        loss, self.step_out = softmax_ce_metrics(logits, labels, self.accum)
        return loss

    def result(self, names: Sequence[str] = ("accuracy",)) -> Dict[str, float]:
        """Means over the steps since ``reset``: ``{"loss": ...}`` plus
        ``"accuracy"`` if it is in ``names``; ``{}`` for no steps. The one
        device-to-host copy. Raises ``ValueError`` if a label was outside
        the class range."""
        loss_sum, acc_sum, steps, bad = self.accum.tolist()
        if bad > 0:
            raise ValueError(
                f"{int(bad)} label(s) outside [0, num_classes) in the last "
                f"{int(steps)} step(s); they were left out of the loss")
        if steps == 0:
            return {}
        out = {"loss": loss_sum / steps}
        if "accuracy" in names:
            out["accuracy"] = acc_sum / steps
        return out
