"""The two callbacks the reference's trainer YAML gives every run (configs/trainer/config.yaml:18-47), for
`mmvae_amd.trainer.Trainer`: `ModelCheckpoint` and `EarlyStopping`, with the argument names and the decision rules of
`lightning.pytorch.callbacks`.  They decide; the Trainer acts (`mmvae_amd.checkpoint.Checkpointer` takes the snapshot).

Monitored values are read from `trainer.callback_metrics`: after a validation the row-weighted epoch mean of every scalar
the validation steps logged (Lightning's `on_epoch=True` reduction), after a training epoch the scalars of its last step.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import List, Optional

_MODES = ("min", "max")


def _better(mode: str, a: float, b: float) -> bool:
    return a < b if mode == "min" else a > b


class Callback:
    """What the Trainer asks of a callback: a name for its entry in the checkpoint and its state."""

    @property
    def state_key(self) -> str:
        return type(self).__name__

    def state_dict(self) -> dict:
        return {}

    def load_state_dict(self, state: dict) -> None:
        pass


class ModelCheckpoint(Callback):
    """`{dirpath}/{filename}.ckpt` whenever `monitor` improves (`save_top_k=1`; without a monitor: at every trigger) and
    `{dirpath}/last.ckpt` at every trigger (`save_last`).  Triggers: the end of a validation -- of every
    `every_n_epochs`-th epoch --, or of the training epoch with `save_on_train_epoch_end`; and every
    `every_n_train_steps` training steps, which writes `last.ckpt` alone (a monitored value belongs to an epoch).
    `dirpath=None`: `<trainer.default_root_dir or the working directory>/checkpoints`.

    `save_top_k` is 0 (no best file) or 1: anything else raises ValueError (Lightning's `-v1` versioning and top-k
    bookkeeping are not built).  The remaining Lightning arguments the reference's YAML lists are accepted and have
    their default meaning only: `save_weights_only=False`, `train_time_interval=None`."""

    def __init__(self, dirpath: Optional[str] = None, filename: Optional[str] = None, monitor: Optional[str] = None,
                 mode: str = "min", save_last: Optional[bool] = None, save_top_k: int = 1,
                 every_n_train_steps: Optional[int] = None, every_n_epochs: Optional[int] = None,
                 save_on_train_epoch_end: Optional[bool] = None, verbose: bool = False, save_weights_only: bool = False,
                 auto_insert_metric_name: bool = True, train_time_interval=None, enable_version_counter: bool = True):
        if save_top_k not in (0, 1):
            raise ValueError(f"ModelCheckpoint: save_top_k={save_top_k!r}; 0 or 1 (top-k bookkeeping is not built)")
        if mode not in _MODES:
            raise ValueError(f"ModelCheckpoint: mode={mode!r}; 'min' or 'max'")
        if save_weights_only:
            raise ValueError("ModelCheckpoint: save_weights_only=True is not built (a checkpoint resumes the run)")
        if train_time_interval is not None:
            raise ValueError("ModelCheckpoint: train_time_interval is not built")
        for name, v in (("every_n_train_steps", every_n_train_steps), ("every_n_epochs", every_n_epochs)):
            if v is not None and int(v) < 0:
                raise ValueError(f"ModelCheckpoint: {name}={v!r}")
        self.dirpath = dirpath
        self.filename = filename or "best_model"
        self.monitor = monitor
        self.mode = mode
        self.save_last = bool(save_last)
        self.save_top_k = int(save_top_k)
        self.every_n_train_steps = int(every_n_train_steps or 0)
        self.every_n_epochs = 1 if every_n_epochs is None else int(every_n_epochs)
        self.save_on_train_epoch_end = bool(save_on_train_epoch_end)
        self.verbose = verbose
        self.best_model_score: Optional[float] = None
        self.best_model_path = ""
        self.last_model_path = ""

    def resolve_dir(self, trainer) -> str:
        if self.dirpath is None:
            self.dirpath = os.path.join(getattr(trainer, "default_root_dir", None) or os.getcwd(), "checkpoints")
        return self.dirpath

    def path(self, trainer, name: str) -> str:
        return os.path.join(self.resolve_dir(trainer), name + ".ckpt")

    def on_train_step(self, trainer) -> List[str]:
        """The files to write behind training step `trainer.global_step` (already counted)."""
        n = self.every_n_train_steps
        if n and trainer.global_step % n == 0 and self.save_last:
            self.last_model_path = self.path(trainer, "last")
            return [self.last_model_path]
        return []

    def on_epoch_trigger(self, trainer, epoch: int, train_epoch_end: bool) -> List[str]:
        """The files to write at the end of epoch `epoch`'s validation (or of its training epoch)."""
        if train_epoch_end != self.save_on_train_epoch_end:
            return []
        if self.every_n_epochs < 1 or (epoch + 1) % self.every_n_epochs:
            return []
        paths = []
        if self.save_top_k == 1:
            if self.monitor is None:
                paths.append(self.path(trainer, self.filename))
            else:
                current = trainer.callback_metrics.get(self.monitor)
                if current is None:
                    raise RuntimeError(f"ModelCheckpoint(monitor={self.monitor!r}): no such logged value; there are "
                                       f"{sorted(trainer.callback_metrics)}")
                current = float(current)
                if not math.isnan(current) and (self.best_model_score is None
                                                or _better(self.mode, current, self.best_model_score)):
                    self.best_model_score = current
                    paths.append(self.path(trainer, self.filename))
            if paths:
                self.best_model_path = paths[0]
        if self.save_last:
            self.last_model_path = self.path(trainer, "last")
            paths.append(self.last_model_path)
        return paths

    def state_dict(self) -> dict:
        return {"monitor": self.monitor, "best_model_score": self.best_model_score, "best_model_path": self.best_model_path,
                "last_model_path": self.last_model_path, "dirpath": self.dirpath}

    def load_state_dict(self, state: dict) -> None:
        self.best_model_score = state.get("best_model_score")
        self.best_model_path = state.get("best_model_path", "")
        self.last_model_path = state.get("last_model_path", "")


class EarlyStopping(Callback):
    """Lightning's rule, checked after every validation: stop when `monitor` is not finite (`check_finite`), has passed
    `stopping_threshold`, is worse than `divergence_threshold`, or has not improved by more than `min_delta` for
    `patience` checks in a row.  `strict`: a monitor that was never logged raises; otherwise it warns and goes on."""

    def __init__(self, monitor: str, min_delta: float = 0.0, patience: int = 3, verbose: bool = False, mode: str = "min",
                 strict: bool = True, check_finite: bool = True, stopping_threshold: Optional[float] = None,
                 divergence_threshold: Optional[float] = None, check_on_train_epoch_end: Optional[bool] = None,
                 log_rank_zero_only: bool = False):
        if mode not in _MODES:
            raise ValueError(f"EarlyStopping: mode={mode!r}; 'min' or 'max'")
        self.monitor = monitor
        self.min_delta = abs(float(min_delta))
        self.patience = int(patience)
        self.mode = mode
        self.strict = strict
        self.check_finite = check_finite
        self.stopping_threshold = None if stopping_threshold is None else float(stopping_threshold)
        self.divergence_threshold = None if divergence_threshold is None else float(divergence_threshold)
        self.check_on_train_epoch_end = bool(check_on_train_epoch_end)
        self.verbose = verbose
        self.wait_count = 0
        self.stopped_epoch = 0
        self.best_score = math.inf if mode == "min" else -math.inf

    def check(self, trainer, epoch: int) -> Optional[str]:
        """The reason to stop after epoch `epoch`, or None."""
        current = trainer.callback_metrics.get(self.monitor)
        if current is None:
            message = (f"EarlyStopping(monitor={self.monitor!r}): no such logged value; there are "
                       f"{sorted(trainer.callback_metrics)}")
            if self.strict:
                raise RuntimeError(message)
            warnings.warn(message)
            return None
        current = float(current)
        reason = None
        if self.check_finite and not math.isfinite(current):
            reason = f"monitored {self.monitor} = {current} is not finite"
        elif self.stopping_threshold is not None and _better(self.mode, current, self.stopping_threshold):
            reason = f"monitored {self.monitor} = {current} passed the stopping threshold {self.stopping_threshold}"
        elif self.divergence_threshold is not None and _better(self.mode, self.divergence_threshold, current):
            reason = f"monitored {self.monitor} = {current} is beyond the divergence threshold {self.divergence_threshold}"
        elif _better(self.mode, current + (self.min_delta if self.mode == "min" else -self.min_delta), self.best_score):
            self.best_score = current
            self.wait_count = 0
        else:
            self.wait_count += 1
            if self.wait_count >= self.patience:
                reason = (f"monitored {self.monitor} did not improve in the last {self.wait_count} checks "
                          f"(best {self.best_score})")
        if reason is not None:
            self.stopped_epoch = epoch
        return reason

    def state_dict(self) -> dict:
        return {"wait_count": self.wait_count, "stopped_epoch": self.stopped_epoch, "best_score": self.best_score,
                "patience": self.patience}

    def load_state_dict(self, state: dict) -> None:
        self.wait_count = state["wait_count"]
        self.stopped_epoch = state["stopped_epoch"]
        self.best_score = state["best_score"]
        self.patience = state["patience"]


# class paths a trainer YAML may name (Trainer.from_yaml) -> the classes above
YAML_CLASS_PATHS = {
    "lightning.pytorch.callbacks.ModelCheckpoint": ModelCheckpoint,
    "lightning.pytorch.callbacks.EarlyStopping": EarlyStopping,
    "mmvae_amd.callbacks.ModelCheckpoint": ModelCheckpoint,
    "mmvae_amd.callbacks.EarlyStopping": EarlyStopping,
}


def from_yaml_list(entries) -> list:
    """The `callbacks:` block of a trainer YAML (a list of {class_path, init_args}) -> callback objects."""
    out = []
    for entry in entries or []:
        cls = YAML_CLASS_PATHS.get(entry.get("class_path"))
        if cls is None:
            raise ValueError(f"trainer YAML: callback {entry.get('class_path')!r} is not one of {sorted(YAML_CLASS_PATHS)}")
        out.append(cls(**(entry.get("init_args") or {})))
    return out
