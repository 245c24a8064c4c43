"""Keras-like ``Model`` facade over a PyTorch-ROCm train loop.

Reference contract (SURVEY.md §2.5 "TF/Keras runtime" row):
``model.compile(optimizer, loss, metrics)`` then
``model.fit(train_ds, steps_per_epoch, epochs, validation_data,
validation_steps, callbacks, verbose)`` -> ``History`` with a ``history``
dict (``Part 1 .../02_model_training_single_node.py:198-215``,
``.../03_model_training_distributed.py:353-370``), and
``model.evaluate(ds, steps)`` -> [loss, accuracy]
(``Part 2 .../01_hyperopt_single_machine_model.py:177``).

``autolog()`` replaces ``mlflow.tensorflow.autolog()``: when enabled, ``fit``
logs params + per-epoch metrics to the active tracking run and the final
model under ``runs:/<id>/model`` (rank 0 only).
"""
from __future__ import annotations

import time
from typing import Dict, Iterable, List, Optional, Sequence, Union

import torch
import torch.nn.functional as F

from ..core import tracking
from ..core.model_io import log_model
from ..utils.trace import ChromeTracer, get_tracer
from .callbacks import Callback, MetricAverageCallback

_autolog_enabled = False


def autolog(enable: bool = True) -> None:
    global _autolog_enabled
    _autolog_enabled = enable


# What ``metrics_on_device=None`` means where the device path is possible.
# Off: on the head-training step the device path's median was 0.045 ms under
# the per-step path's, inside that contender's spread of 0.379 ms, so the
# routing rule does not keep it as the default (docs/KERNELS.md, "Benchmark:
# the facade and the optimizer step"). ``metrics_on_device=True`` asks for it.
_DEVICE_METRICS_DEFAULT = False

# optimizer names with a fused, fp32-master kernel (ops/optim.py)
_FUSED_NAMES = ("adam", "sgd", "adadelta")


def _make_optimizer(spec, params, lr: Optional[float] = None,
                    precision: str = "fp32"):
    if isinstance(spec, torch.optim.Optimizer):
        return spec
    from ..parallel.api import DistributedOptimizer

    if isinstance(spec, DistributedOptimizer):
        return spec
    name = str(spec)
    if precision == "bf16" and name.lower() not in _FUSED_NAMES:
        # a stock optimizer would keep state and update in bf16 and round
        # most small updates away
        raise ValueError(
            f"optimizer {spec!r} has no fp32-master kernel for precision="
            "'bf16'; use one of 'Adam', 'SGD', 'Adadelta' or pass an "
            "optimizer instance")
    lr = 1e-3 if lr is None else lr
    key = name.lower()
    params = list(params)
    # fused ddlw optimizers on GPU (K10); stock torch otherwise
    on_gpu = bool(params) and params[0].is_cuda
    if on_gpu and key in _FUSED_NAMES:
        from ..ops.optim import FusedAdadelta, FusedAdam, FusedSGD

        if key == "adam":
            return FusedAdam(params, lr=lr)
        if key == "adadelta":
            return FusedAdadelta(params, lr=lr)
        return FusedSGD(params, lr=lr, momentum=0.0)
    table = {
        "adam": torch.optim.Adam,
        "adadelta": torch.optim.Adadelta,
        "sgd": torch.optim.SGD,
        "adamw": torch.optim.AdamW,
    }
    if key not in table:
        raise ValueError(f"unknown optimizer {spec!r}")
    return table[key](params, lr=lr)


def sparse_categorical_crossentropy_from_logits(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The reference's loss (``.../02_model_training_single_node.py:202``);
    fused HIP kernel (K9) on GPU, stock cross_entropy on CPU."""
    from ..ops.layers import softmax_cross_entropy

    return softmax_cross_entropy(logits, labels)


class History:
    def __init__(self):
        self.history: Dict[str, List[float]] = {}

    def _append(self, logs: Dict[str, float]) -> None:
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


def _accuracy(logits, labels):
    """K11 on the hip kernel for CUDA logits; torch ops otherwise."""
    if logits.is_cuda and logits.dim() == 2:
        try:
            from ..ops import binding

            return binding.accuracy(logits, labels)
        except Exception:
            pass
    return (logits.argmax(-1) == labels).float().mean()


class _RunAhead:
    """Bound on how far the host runs ahead of the device when no step reads
    anything back. ``tick()`` after a step records an event and waits for the
    one recorded ``depth - 1`` steps before it, so when the next step is
    issued at most ``depth`` steps are unfinished. The events are recorded
    on ``device``'s current stream, whichever device is current, and are made
    once: ``reset()`` starts a new loop on the same ring."""

    def __init__(self, depth: int, device):
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.events = [torch.cuda.Event() for _ in range(depth)]
        self.n = 0

    def reset(self) -> None:
        self.n = 0

    def tick(self) -> None:
        d = len(self.events)
        self.events[self.n % d].record(torch.cuda.current_stream(self.device))
        self.n += 1
        if self.n >= d:
            self.events[self.n % d].synchronize()


class Model:
    """Wraps an ``nn.Module`` with compile/fit/evaluate.

    ``precision``:

    - ``"fp32"`` (default): the module and the batches are used as given.
    - ``"bf16"``: the state the hand-written kernels are gated on. Needs a
      CUDA device. The module is moved there and ``ops.apply_bf16_policy``
      applied here, before any optimizer can be built from the parameters;
      every batch goes through ``ops.prepare_batch`` (uint8 N x H x W x C
      from the loader is the fast door); ``compile`` with an optimizer name
      gives an fp32-master fused optimizer; ``predict`` returns fp32 logits.
    - ``"auto"``: ``"bf16"`` on a CUDA device with the kernel library
      loadable, else ``"fp32"``.

    The resolved value is ``model.precision``. Saving is unchanged: under
    bf16 the conv and linear weights are stored as bf16; ``load_model``
    rebuilds the module in fp32 and ``load_state_dict`` widens them exactly.
    The policy is not persisted — pass ``precision`` again after loading.

    ``RUN_AHEAD`` (2): with the metrics on the device no step reads anything
    back, so nothing else stops the host from queueing a whole epoch of an
    in-memory dataset. ``fit`` and ``evaluate`` let at most this many steps
    be unfinished when they issue the next one. Two is the least that keeps
    the device busy: one step runs while the host queues the one after it. A
    deeper queue hides nothing more, because a step is queued no faster than
    the launch rate that already bounds it, and it delays ``stop_training``,
    an interrupt and the epoch's clock by as many steps.
    """

    RUN_AHEAD = 2

    def __init__(self, module: torch.nn.Module, device: Optional[torch.device] = None,
                 precision: str = "fp32"):
        self.module = module
        if device is None:
            try:
                device = next(module.parameters()).device
            except StopIteration:
                device = torch.device("cpu")
        self.device = device
        if precision not in ("fp32", "bf16", "auto"):
            raise ValueError(
                f"precision must be 'fp32', 'bf16' or 'auto', got {precision!r}")
        on_cuda = torch.device(device).type == "cuda"
        if precision == "auto":
            from ..ops import has_lib

            precision = "bf16" if on_cuda and has_lib() else "fp32"
        elif precision == "bf16" and not on_cuda:
            raise ValueError(
                f"precision='bf16' needs a CUDA device, got {device}")
        self.precision = precision
        if precision == "bf16":
            from ..ops.precision import apply_bf16_policy

            self.module = apply_bf16_policy(module.to(device))
        self.optimizer = None
        self.loss_fn = sparse_categorical_crossentropy_from_logits
        self.metrics: Sequence[str] = ()
        self.stop_training = False
        self._steps_per_epoch: Optional[int] = None
        self._train_metrics = None
        self._eval_metrics = None
        self._ahead = None

    # the running sums of the ``*_step_async`` methods, made on first use
    @property
    def train_metrics(self):
        if self._train_metrics is None:
            from .metrics import DeviceMetrics

            self._train_metrics = DeviceMetrics(self.device)
        return self._train_metrics

    @property
    def eval_metrics(self):
        if self._eval_metrics is None:
            from .metrics import DeviceMetrics

            self._eval_metrics = DeviceMetrics(self.device)
        return self._eval_metrics

    # ------------------------------------------------------------------ #
    def compile(
        self,
        optimizer: Union[str, torch.optim.Optimizer] = "Adam",
        loss=None,
        metrics: Sequence[str] = ("accuracy",),
        learning_rate: Optional[float] = None,
    ) -> "Model":
        trainable = [p for p in self.module.parameters() if p.requires_grad]
        self.optimizer = _make_optimizer(optimizer, trainable, learning_rate,
                                         self.precision)
        if loss is not None:
            self.loss_fn = loss
        self.metrics = tuple(metrics)
        return self

    # ------------------------------------------------------------------ #
    def _move(self, x: torch.Tensor) -> torch.Tensor:
        return x.to(self.device, non_blocking=True) if x.device != self.device else x

    def _images(self, x: torch.Tensor) -> torch.Tensor:
        """Batch to the device and, under bf16, into the policy's layout."""
        x = self._move(x)
        if self.precision == "bf16":
            from ..ops.precision import prepare_batch

            x = prepare_batch(self.module, x)
        return x

    def _forward_loss(self, images: torch.Tensor, labels: torch.Tensor):
        logits = self.module(images)
        loss = self.loss_fn(logits, labels)
        return logits, loss

    def train_step(self, images: torch.Tensor, labels: torch.Tensor) -> Dict[str, float]:
        self.module.train()
        images, labels = self._images(images), self._move(labels)
        self.optimizer.zero_grad(set_to_none=True)
        logits, loss = self._forward_loss(images, labels)
        loss.backward()
        self.optimizer.step()
        out = {"loss": float(loss.detach())}
        if "accuracy" in self.metrics:
            out["accuracy"] = float(_accuracy(logits.detach(), labels))
        return out

    @torch.no_grad()
    def eval_step(self, images: torch.Tensor, labels: torch.Tensor) -> Dict[str, float]:
        self.module.eval()
        images, labels = self._images(images), self._move(labels)
        logits, loss = self._forward_loss(images, labels)
        out = {"loss": float(loss)}
        if "accuracy" in self.metrics:
            out["accuracy"] = float(_accuracy(logits, labels))
        return out

    def train_step_async(self, images: torch.Tensor, labels: torch.Tensor) -> None:
        """``train_step`` with nothing read back: loss, gradient, accuracy
        and the running sums come from one kernel (``train_metrics``), so the
        call returns once the step is queued."""
        self.module.train()
        images, labels = self._images(images), self._move(labels)
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.train_metrics.update(self.module(images), labels)
        loss.backward()
        self.optimizer.step()

    @torch.no_grad()
    def eval_step_async(self, images: torch.Tensor, labels: torch.Tensor) -> None:
        """``eval_step`` with nothing read back (``eval_metrics``)."""
        self.module.eval()
        images, labels = self._images(images), self._move(labels)
        self.eval_metrics.update(self.module(images), labels)

    def _run_ahead(self) -> _RunAhead:
        """This model's run-ahead bound, restarted for a new step loop."""
        if self._ahead is None or len(self._ahead.events) != self.RUN_AHEAD:
            self._ahead = _RunAhead(self.RUN_AHEAD, self.device)
        self._ahead.reset()
        return self._ahead

    # ------------------------------------------------------------------ #
    def _device_metrics_blocker(self, callbacks: Sequence[Callback]) -> Optional[str]:
        """Why ``fit`` / ``evaluate`` cannot keep the metrics on the device,
        or None if they can."""
        from ..ops import has_lib
        from ..ops.layers import _hip_ops_disabled

        if torch.device(self.device).type != "cuda":
            return f"the model is on {self.device}, not on a CUDA device"
        if _hip_ops_disabled():
            return "DDLW_DISABLE_HIP_OPS=1 switches the kernels off"
        if not has_lib():
            return "the kernel library is not loadable"
        if self.loss_fn is not sparse_categorical_crossentropy_from_logits:
            return "the loss is not the default sparse_categorical_crossentropy_from_logits"
        extra = [m for m in self.metrics if m != "accuracy"]
        if extra:
            return f"metrics {extra} are not computed on the device (only 'accuracy')"
        for cb in callbacks:
            if type(cb).on_batch_end is not Callback.on_batch_end:
                return (f"callback {type(cb).__name__} overrides on_batch_end "
                        "and needs the logs of every step")
        return None

    def _use_device_metrics(self, flag: Optional[bool],
                            callbacks: Sequence[Callback] = ()) -> bool:
        if flag is False or (flag is None and not _DEVICE_METRICS_DEFAULT):
            return False
        why = self._device_metrics_blocker(callbacks)
        if flag and why is not None:
            raise ValueError(f"metrics_on_device=True, but {why}")
        return why is None

    # ------------------------------------------------------------------ #
    def fit(
        self,
        data: Iterable,
        steps_per_epoch: Optional[int] = None,
        epochs: int = 1,
        validation_data: Optional[Iterable] = None,
        validation_steps: Optional[int] = None,
        callbacks: Sequence[Callback] = (),
        verbose: int = 1,
        metrics_on_device: Optional[bool] = None,
    ) -> History:
        """``metrics_on_device``: ``True`` keeps loss and accuracy on the
        device and reads them once per epoch; it raises ``ValueError`` naming
        the reason where that is not possible (it needs CUDA, the kernels
        on, the default loss, no metric but accuracy and no callback that
        overrides ``on_batch_end``). ``False`` reads them back every step.
        ``None`` is auto: the device path where it is possible and
        ``_DEVICE_METRICS_DEFAULT`` holds — which it does not as shipped,
        the measured gain being inside the spread, so ``None`` is ``False``
        today. The validation pass gets the same value and decides for
        itself: it has no callbacks, so a callback that holds training on
        the per-step path does not hold validation there."""
        if self.optimizer is None:
            raise RuntimeError("call compile() before fit()")
        on_device = self._use_device_metrics(metrics_on_device, callbacks)
        # An infinite stream (Petastorm num_epochs=None semantics) with no
        # steps_per_epoch would never end an epoch — fail loudly instead
        # (Keras shares this footgun; we don't).
        if steps_per_epoch is None and getattr(data, "num_epochs", 0) is None:
            raise ValueError(
                "fit(): dataset advertises infinite epochs (num_epochs=None) "
                "but steps_per_epoch was not given — the first epoch would "
                "never end. Pass steps_per_epoch (e.g. len(converter) // "
                "(batch_size * size()))."
            )
        from ..parallel import api

        self.stop_training = False
        self._steps_per_epoch = steps_per_epoch
        history = History()
        # MetricAverage must run before LR-schedule callbacks (reference
        # comment .../03_model_training_distributed.py:310-313): stable-sort
        # metric-average callbacks to the front.
        callbacks = sorted(
            callbacks, key=lambda c: 0 if isinstance(c, MetricAverageCallback) else 1
        )
        for cb in callbacks:
            cb.set_model(self)
        for cb in callbacks:
            cb.on_train_begin()

        run = tracking.active_run() if _autolog_enabled else None
        if run is not None and api.rank() == 0:
            run.log_params(
                {
                    "optimizer_name": type(self.optimizer).__name__,
                    "learning_rate": self.optimizer.param_groups[0]["lr"],
                    "epochs": epochs,
                    "steps_per_epoch": steps_per_epoch or -1,
                    "precision": self.precision,
                }
            )

        # Horovod-Timeline equivalent: DDLW_TIMELINE=<path> -> chrome trace
        from ..parallel import api as _api

        tracer = get_tracer()
        data_iter = iter(data)
        for epoch in range(epochs):
            for cb in callbacks:
                cb.on_epoch_begin(epoch)
            t0 = time.time()
            agg: Dict[str, float] = {}
            n = 0
            step = 0
            if on_device:
                self.train_metrics.reset()
                ahead = self._run_ahead()
            while steps_per_epoch is None or step < steps_per_epoch:
                with tracer.span(f"data[e{epoch}s{step}]", "data", tid=_api.rank()):
                    try:
                        images, labels = next(data_iter)
                    except StopIteration:
                        if steps_per_epoch is None:
                            data_iter = iter(data)  # next epoch restarts iterator
                            break
                        data_iter = iter(data)
                        try:
                            images, labels = next(data_iter)
                        except StopIteration:
                            break
                for cb in callbacks:
                    cb.on_batch_begin(step)
                if on_device:
                    # no callback here overrides on_batch_end: nothing to call
                    with tracer.span(f"train_step[e{epoch}s{step}]", "step", tid=_api.rank()):
                        self.train_step_async(images, labels)
                    ahead.tick()
                    step += 1
                    continue
                with tracer.span(f"train_step[e{epoch}s{step}]", "step", tid=_api.rank()):
                    logs = self.train_step(images, labels)
                for cb in callbacks:
                    cb.on_batch_end(step, logs)
                for k, v in logs.items():
                    agg[k] = agg.get(k, 0.0) + v
                n += 1
                step += 1
            if on_device:
                epoch_logs = self.train_metrics.result(self.metrics)
            else:
                epoch_logs = {k: v / max(n, 1) for k, v in agg.items()}

            if validation_data is not None:
                val_logs = self.evaluate(
                    validation_data, steps=validation_steps, return_dict=True,
                    metrics_on_device=metrics_on_device,
                )
                epoch_logs.update({f"val_{k}": v for k, v in val_logs.items()})

            for cb in callbacks:
                cb.on_epoch_end(epoch, epoch_logs)
            history._append(epoch_logs)
            if run is not None and api.rank() == 0:
                run.log_metrics(epoch_logs, step=epoch)
            if verbose and api.rank() == 0:
                msg = " - ".join(f"{k}: {v:.4f}" for k, v in epoch_logs.items())
                print(f"Epoch {epoch + 1}/{epochs} [{time.time() - t0:.1f}s] {msg}", flush=True)
            if self.stop_training:
                break

        for cb in callbacks:
            cb.on_train_end()
        tracer.save()
        if run is not None and api.rank() == 0:
            log_model(self.module, "model")
        return history

    # ------------------------------------------------------------------ #
    def evaluate(
        self,
        data: Iterable,
        steps: Optional[int] = None,
        return_dict: bool = False,
        metrics_on_device: Optional[bool] = None,
    ):
        """``metrics_on_device``: as for ``fit``; one readback per call."""
        on_device = self._use_device_metrics(metrics_on_device)
        agg: Dict[str, float] = {}
        n = 0
        it = iter(data)
        step = 0
        if on_device:
            self.eval_metrics.reset()
            ahead = self._run_ahead()
        while steps is None or step < steps:
            try:
                images, labels = next(it)
            except StopIteration:
                break
            if on_device:
                self.eval_step_async(images, labels)
                ahead.tick()
                step += 1
                continue
            logs = self.eval_step(images, labels)
            for k, v in logs.items():
                agg[k] = agg.get(k, 0.0) + v
            n += 1
            step += 1
        if on_device:
            out = self.eval_metrics.result(self.metrics)
        else:
            out = {k: v / max(n, 1) for k, v in agg.items()}
        if return_dict:
            return out
        return [out.get("loss", 0.0)] + [out[m] for m in self.metrics if m in out]

    @torch.no_grad()
    def predict(self, images: torch.Tensor, batch_size: int = 128) -> torch.Tensor:
        self.module.eval()
        outs = []
        for i in range(0, len(images), batch_size):
            logits = self.module(self._images(images[i : i + batch_size]))
            if self.precision == "bf16":
                logits = logits.float()  # on the device: numpy has no bf16
            outs.append(logits.cpu())
        return torch.cat(outs)
