"""Minimal fit / validate / predict loop for CMMVAEModel when Lightning is not installed.

Stands in for the part of `lightning.pytorch.Trainer` the reference's trainer YAML exercises (configs/trainer/config.yaml:
max_epochs / max_steps / limit_*_batches / check_val_every_n_epoch / num_sanity_val_steps) -- manual optimisation, so
the loop only sets the stage flags and calls the step methods.  Batches are `(x, metadata, expert_id)` tuples as
produced by the reference's datamodules (data/local/cellxgene_manager.py:76-88); `MultiModalBatches` below mirrors
`MultiModalDataLoader` (data/local/multi_modal_loader.py:36-68) with a seeded, rank-synchronous modality choice.
"""
from __future__ import annotations

import random
from typing import Dict, Iterable, Iterator, List, Optional

import torch
import yaml


class MultiModalBatches:
    """Interleaves per-modality batch iterables: at every step one modality that still has batches is drawn (seeded
    `random.Random`, identical on every rank so that data-parallel ranks train the same expert)."""

    def __init__(self, loaders: Dict[str, Iterable], seed: int = 0, round_robin: bool = False):
        self.loaders = loaders
        self.seed = seed
        self.round_robin = round_robin
        self.epoch = 0

    def __iter__(self) -> Iterator:
        rng = random.Random(self.seed + self.epoch)
        self.epoch += 1
        its = {k: iter(v) for k, v in self.loaders.items()}
        order: List[str] = list(its.keys())
        i = 0
        while its:
            key = order[i % len(order)] if self.round_robin else rng.choice(sorted(its.keys()))
            i += 1
            if key not in its:
                continue
            try:
                yield next(its[key])
            except StopIteration:
                del its[key]
                order = [k for k in order if k in its]


class Lookahead:
    """Wraps a batch iterable and tells the model, before each batch is handed out, which batch comes AFTER it
    (`CMMVAEModel.hint_next_batch`): the step engine then computes the next step's first forward product beside the
    current step's forward chain (software pipelining across steps).  Works around any loop that pulls batches one at a
    time -- this module's Trainer, or a Lightning Trainer given `Lookahead(dataloader, model)` as its train dataloader.
    A consumer that stops early (break, limit_train_batches) leaves a batch announced that will never be trained: the
    iterator withdraws it when it is closed (`CMMVAEModel.withdraw_hint`; a model without it is told None) -- at the
    `break` under CPython's reference counting, and when the batches themselves raise.  When the CONSUMER's step raises,
    the traceback keeps the iterator alive and the withdrawal waits for the exception's release: a loop that catches the
    error and goes on calls `withdraw_hint()` itself (the engine's identity check holds either way)."""

    def __init__(self, batches: Iterable, model):
        self.batches, self.model = batches, model

    def __len__(self):
        return len(self.batches)

    def __iter__(self) -> Iterator:
        it = iter(self.batches)
        try:
            cur = next(it)
        except StopIteration:
            return
        exhausted = False
        try:
            for nxt in it:
                self.model.hint_next_batch(nxt)
                yield cur
                cur = nxt
            self.model.hint_next_batch(None)
            yield cur
            exhausted = True
        finally:
            if not exhausted:  # (GeneratorExit at a yield: the consumer stopped; or the batches raised)
                withdraw = getattr(self.model, "withdraw_hint", None)
                withdraw() if withdraw is not None else self.model.hint_next_batch(None)


class _SkipFirst:
    """`batches` without its first `n` (a resumed epoch: what the interrupted run had already consumed is drawn and
    dropped, so that the modality draws and the loaders stand where they stood)."""

    def __init__(self, batches: Iterable, n: int):
        self.batches, self.n = batches, n

    def __iter__(self) -> Iterator:
        it = iter(self.batches)
        for _ in range(self.n):
            if next(it, None) is None:
                return
        yield from it


def _epoch_source(batches) -> Optional[MultiModalBatches]:
    """The MultiModalBatches behind `batches` (itself, or wrapped in a Prefetcher / Lookahead): its `epoch` seeds the
    modality draws, so a checkpoint records it."""
    for _ in range(4):
        if isinstance(batches, MultiModalBatches):
            return batches
        batches = getattr(batches, "batches", None)
        if batches is None:
            break
    return None


class Trainer:
    def __init__(self, max_epochs: int = 10, max_steps: int = -1, limit_train_batches: Optional[int] = None,
                 limit_val_batches: Optional[int] = None, check_val_every_n_epoch: int = 1,
                 num_sanity_val_steps: int = 0, callbacks: Optional[list] = None, default_root_dir: Optional[str] = None,
                 enable_checkpointing: bool = True, **unused):
        """callbacks: `mmvae_amd.callbacks.ModelCheckpoint` / `EarlyStopping` objects (at most one ModelCheckpoint); with
        none, fit() does what it did before there were any.  default_root_dir: where a ModelCheckpoint without a dirpath
        puts `checkpoints/`.  enable_checkpointing=False with a ModelCheckpoint among the callbacks raises, as in
        Lightning."""
        from .callbacks import EarlyStopping, ModelCheckpoint

        self.max_epochs = max_epochs
        self.max_steps = max_steps
        self.limit_train_batches = limit_train_batches
        self.limit_val_batches = limit_val_batches
        self.check_val_every_n_epoch = check_val_every_n_epoch
        self.num_sanity_val_steps = num_sanity_val_steps
        self.global_step = 0
        self.history: List[dict] = []
        self.callbacks = list(callbacks or [])
        self.default_root_dir = default_root_dir
        self.enable_checkpointing = enable_checkpointing
        ckpts = [c for c in self.callbacks if isinstance(c, ModelCheckpoint)]
        if len(ckpts) > 1:
            raise ValueError("Trainer: one ModelCheckpoint at most (a second one would need a second snapshot buffer)")
        if ckpts and not enable_checkpointing:
            raise ValueError("Trainer: enable_checkpointing=False, but a ModelCheckpoint is among the callbacks")
        self.checkpoint_callback = ckpts[0] if ckpts else None
        self.early_stopping_callbacks = [c for c in self.callbacks if isinstance(c, EarlyStopping)]
        self.callback_metrics: Dict[str, float] = {}  # what the callbacks monitor (mmvae_amd.callbacks)
        self.current_epoch = 0
        self.should_stop = False
        self.stop_reason: Optional[str] = None
        self.checkpointer = None  # mmvae_amd.checkpoint.Checkpointer of the model being fitted
        self._pending = None  # the save in flight
        self._diverged = False  # a snapshot found non-finite values: nothing more is written
        self._resume: Optional[dict] = None  # position in the data a loaded checkpoint asks fit() to take up

    @classmethod
    def from_yaml(cls, path: str) -> "Trainer":
        from .callbacks import from_yaml_list

        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
        keys = ("max_epochs", "max_steps", "limit_train_batches", "limit_val_batches", "check_val_every_n_epoch",
                "num_sanity_val_steps", "default_root_dir", "enable_checkpointing")
        kw = {k: cfg[k] for k in keys if cfg.get(k) is not None}
        if cfg.get("callbacks"):
            kw["callbacks"] = from_yaml_list(cfg["callbacks"])
        return cls(**kw)

    def _snapshot(self, model) -> dict:
        return {k: (float(v.detach()) if torch.is_tensor(v) else v) for k, v in model.logged.items()}

    def fit(self, model, train_batches: Iterable, val_batches: Optional[Iterable] = None,
            ckpt_path: Optional[str] = None):
        """ckpt_path: a file written by this Trainer's ModelCheckpoint (mmvae_amd.checkpoint): the model, the optimisers,
        the random state, `global_step`, the epoch, the callbacks' state and `history` are restored and the run goes on
        where the file was written -- for a mid-epoch file behind the batches that epoch had already consumed.  With
        callbacks, `stop_reason` says afterwards why the run ended early (None: it did not), and the last checkpoint
        write has finished when fit() returns."""
        model.optimizers()
        stub = model.trainer
        self.should_stop, self.stop_reason, self._diverged = False, None, False
        if self.checkpoint_callback is not None and self.checkpointer is None:
            from .checkpoint import Checkpointer

            self.checkpointer = Checkpointer(model)  # (buffers and job table: once, before the first captured step)
        if ckpt_path is not None:
            from .checkpoint import load

            load(ckpt_path, model, trainer=self)
            stub.global_step = self.global_step
        resume, self._resume = self._resume or {}, None
        source, val_source = _epoch_source(train_batches), _epoch_source(val_batches)
        if source is not None and resume.get("batches_epoch") is not None:
            source.epoch = resume["batches_epoch"]
        if val_source is not None and resume.get("val_batches_epoch") is not None:
            val_source.epoch = resume["val_batches_epoch"]
        skip = int(resume.get("batches_consumed") or 0)
        for epoch in range(int(resume.get("next_epoch") or 0), self.max_epochs):
            self.current_epoch = epoch
            seed_epoch = source.epoch if source is not None else None  # (what this epoch's modality draws are seeded with)
            model.train()
            stub.set_stage("training")
            batches = _SkipFirst(train_batches, skip) if skip else train_batches
            for i, batch in enumerate(Lookahead(batches, model) if hasattr(model, "hint_next_batch") else batches, start=skip):
                if self.limit_train_batches is not None and i >= self.limit_train_batches:
                    break
                model.training_step(batch, i)
                self.global_step += 1
                stub.global_step = self.global_step
                if self.checkpoint_callback is not None:
                    paths = self.checkpoint_callback.on_train_step(self)
                    if paths:
                        self._save(model, paths, epoch, {"next_epoch": epoch, "batches_consumed": i + 1,
                                                         "batches_epoch": seed_epoch,
                                                         "val_batches_epoch": getattr(val_source, "epoch", None)})
                    if self._pending is not None and self._pending.done():
                        self._settle_pending()  # (a finished write: a refusal for non-finite values ends the run here)
                    if self.should_stop:
                        break
                if 0 < self.max_steps <= self.global_step:
                    break
            skip = 0
            self.history.append({"epoch": epoch, "stage": "training", **self._snapshot(model)})
            if self.callbacks:
                self.callback_metrics.update({k: v for k, v in self.history[-1].items() if isinstance(v, float)})
                self._epoch_callbacks(model, epoch, seed_epoch, val_source, train_epoch_end=True)
                if val_batches is None:  # (no validation: its callbacks act on the training epoch's values, as in Lightning)
                    self._epoch_callbacks(model, epoch, seed_epoch, val_source, train_epoch_end=False)
            if val_batches is not None and (epoch + 1) % self.check_val_every_n_epoch == 0 and not self.should_stop:
                self.validate(model, val_batches)
                if self.callbacks:
                    self._epoch_callbacks(model, epoch, seed_epoch, val_source, train_epoch_end=False)
            if 0 < self.max_steps <= self.global_step or self.should_stop:
                break
        self._finish_saves()
        return self.history

    # ------------------------------------------------------------------------------------------------- callbacks
    def _epoch_callbacks(self, model, epoch: int, seed_epoch, val_source, train_epoch_end: bool) -> None:
        """Behind a training epoch / a validation: the early-stopping checks, then the checkpoint the ModelCheckpoint asks
        for (Lightning's order: the file holds the early-stopping state of the check just made; the epoch that stops the
        run is still saved)."""
        position = {"next_epoch": epoch + 1, "batches_consumed": 0,
                    "batches_epoch": None if seed_epoch is None else seed_epoch + 1,
                    "val_batches_epoch": getattr(val_source, "epoch", None)}
        for stopper in self.early_stopping_callbacks:
            if stopper.check_on_train_epoch_end == train_epoch_end:
                reason = stopper.check(self, epoch)
                if reason is not None:
                    self.should_stop, self.stop_reason = True, self.stop_reason or reason
        if self.checkpoint_callback is not None:
            paths = self.checkpoint_callback.on_epoch_trigger(self, epoch, train_epoch_end)
            if paths:
                self._save(model, paths, epoch, position)

    def _save(self, model, paths: List[str], epoch: int, position: dict) -> None:
        """One snapshot into every path of `paths`.  The save before it is looked at first: had it found non-finite
        values, its files were left as they were, the run stops and nothing more is written."""
        if self._settle_pending():
            return
        extra = {"epoch": epoch, "global_step": self.global_step,
                 "callbacks": {c.state_key: c.state_dict() for c in self.callbacks},
                 "mmvae_amd": {**position, "history": self.history}}
        self._pending = self.checkpointer.save(paths[0], extra, also=paths[1:])

    def _settle_pending(self) -> bool:
        """Wait for the save in flight (its error is raised here).  True when it refused to write: non-finite values."""
        pending, self._pending = self._pending, None
        if pending is None:
            return self._diverged
        pending.wait()
        if pending.nonfinite:
            self.should_stop = self._diverged = True
            self.stop_reason = (f"checkpoint not written: non-finite values in {sorted(pending.nonfinite)} "
                                f"(global step {self.global_step})")
            return True
        return False

    def _finish_saves(self) -> None:
        self._settle_pending()
        if self.checkpointer is not None:
            self.checkpointer.wait()

    def _resume_from(self, ckpt: dict) -> None:
        """mmvae_amd.checkpoint.load(..., trainer=self): take up the file's position."""
        own = ckpt["mmvae_amd"]
        self.global_step = int(ckpt["global_step"])
        self.current_epoch = int(own.get("next_epoch") or 0)
        self.history = list(own.get("history") or [])
        states = ckpt.get("callbacks") or {}
        for c in self.callbacks:
            if c.state_key in states:
                c.load_state_dict(states[c.state_key])
        self._resume = {k: own.get(k) for k in ("next_epoch", "batches_consumed", "batches_epoch", "val_batches_epoch")}

    @torch.no_grad()
    def validate(self, model, batches: Iterable):
        model.eval()
        model.trainer.set_stage("validation")
        sums: dict = {}
        for i, batch in enumerate(batches):
            if self.limit_val_batches is not None and i >= self.limit_val_batches:
                break
            model.validation_step(batch, i)
            if self.callbacks:
                self._accumulate(model, batch, sums)
        self.history.append({"stage": "validation", **self._snapshot(model)})
        if self.callbacks:
            self._reduce(sums)

    @staticmethod
    def _accumulate(model, batch, sums: dict) -> None:
        """The scalars this validation step logged (`.../validation/<expert>` and `val_loss`), times the batch's rows,
        added to the epoch's sums where they are: device scalars stay on the device, nothing is read here."""
        rows = int(batch[0].shape[0])
        suffix = f"/validation/{batch[2]}"
        for key, v in model.logged.items():
            if not (key.endswith(suffix) or key == "val_loss"):
                continue
            term = v.detach() * rows if torch.is_tensor(v) else float(v) * rows
            held = sums.get(key)
            sums[key] = (term, rows) if held is None else (held[0] + term, held[1] + rows)

    def _reduce(self, sums: dict) -> None:
        """Row-weighted epoch means -> callback_metrics, with ONE read of the device sums."""
        on_device = [k for k, (t, _) in sums.items() if torch.is_tensor(t)]
        if on_device:
            host = torch.stack([sums[k][0].reshape(()).float() for k in on_device]).cpu().tolist()
            for k, v in zip(on_device, host):
                self.callback_metrics[k] = v / sums[k][1]
        for k, (t, rows) in sums.items():
            if not torch.is_tensor(t):
                self.callback_metrics[k] = t / rows

    @torch.no_grad()
    def predict(self, model, batches: Iterable, writer=None) -> list:
        """`predict_step` over the batches; with a `mmvae_amd.predictions.PredictionWriter` every batch is appended
        to `predictions.h5` as it is produced (the reference's write_interval="batch" callback) and nothing is kept."""
        model.eval()
        model.trainer.set_stage("prediction")
        if writer is None:
            return [model.predict_step(batch, i) for i, batch in enumerate(batches)]
        writer.on_predict_start(self, model)
        for i, batch in enumerate(batches):
            writer.write_on_batch_end(self, model, model.predict_step(batch, i), None, batch, i, 0)
        writer.on_predict_epoch_end(self, model)
        return []

    @torch.no_grad()
    def cross_generate(self, model, batches: Iterable, targets=None, writer=None) -> list:
        """`cross_generate_step` over the batches, like predict(): eval mode, stage "prediction"; with a
        PredictionWriter every batch's z and xhat_<target> matrices are appended to predictions.h5 and nothing is kept."""
        model.eval()
        model.trainer.set_stage("prediction")
        if writer is None:
            return [model.cross_generate_step(batch, i, targets=targets) for i, batch in enumerate(batches)]
        writer.on_predict_start(self, model)
        for i, batch in enumerate(batches):
            writer.write_on_batch_end(self, model, model.cross_generate_step(batch, i, targets=targets), None, batch, i, 0)
        writer.on_predict_epoch_end(self, model)
        return []

    @torch.no_grad()
    def umap(self, model, batches: Iterable, **kw):
        """(embedding [cells, n_components], metadata) of the UMAP of the latent embeddings: `predict_step` over the
        batches with z kept where it was produced, then `mmvae_amd.umap.umap_embeddings(z, **kw)` (the reference's
        runners/umap_predictions.py:25-50, there on the host from predictions.h5).  metadata is the batches' frames
        stacked, one row per cell, with the "species" column predict_step adds;
        `predictions.write_umap_embeddings` stores the embedding next to the predictions."""
        import pandas as pd

        from .constants import REGISTRY_KEYS as RK
        from .umap import umap_embeddings

        outs = [p[RK.Z] for p in self.predict(model, batches)]
        if not outs:
            raise ValueError("Trainer.umap: no batches")
        z = torch.cat([o[0] for o in outs], 0)
        metadata = pd.concat([o[1] for o in outs], ignore_index=True)
        return umap_embeddings(z, **kw), metadata

    @torch.no_grad()
    def umap_plots(self, model, batches: Iterable, categories, save_dir: str, key: str = "z", n_largest: int = 15,
                   method: str = "", plot_kw: Optional[dict] = None, **umap_kw) -> List[str]:
        """`Trainer.umap`, then one `mmvae_amd.plots.plot_category` per category of `categories` (columns of the batches'
        metadata): the files `save_dir`/integrated.{category}.umap.{key}.png, whose paths are returned.  The embedding
        stays on the device until its raster has been made there; what reaches the host is the picture.  `plot_kw` goes to
        plot_category (alpha, marker_size, decorate, colors, ...), every further keyword to `umap_embeddings`."""
        from .plots import plot_category

        embedding, metadata = self.umap(model, batches, **umap_kw)
        return [plot_category(embedding, metadata, category, save_dir, n_largest, key, method, **(plot_kw or {}))
                for category in categories]

    @torch.no_grad()
    def integration_metrics(self, model, batches: Iterable, **kw):
        """`mmvae_amd.mixing.integration_metrics` of the latent embeddings: `predict_step` over the batches with z kept
        where it was produced, the batches' metadata frames stacked (one row per cell, with the "species" column
        predict_step adds -- the default batch column), then LISI of the batch and label columns and the label transfer
        across the batches on the exact kNN graph of z.  `kw`: batch_key, label_keys, n_neighbors, perplexity, transfer."""
        import pandas as pd

        from .constants import REGISTRY_KEYS as RK
        from .mixing import integration_metrics

        outs = [p[RK.Z] for p in self.predict(model, batches)]
        if not outs:
            raise ValueError("Trainer.integration_metrics: no batches")
        z = torch.cat([o[0] for o in outs], 0)
        metadata = pd.concat([o[1] for o in outs], ignore_index=True)
        return integration_metrics(z, metadata, **kw)

    @torch.no_grad()
    def silhouette_widths(self, model, batches: Iterable, **kw):
        """`mmvae_amd.silhouette.silhouette_widths` of the latent embeddings: z and the metadata gathered exactly as
        `integration_metrics` gathers them, then the label silhouette of every label column and the batch silhouette
        inside its classes, over all cells.  `kw`: batch_key, label_keys, metric."""
        import pandas as pd

        from .constants import REGISTRY_KEYS as RK
        from .silhouette import silhouette_widths

        outs = [p[RK.Z] for p in self.predict(model, batches)]
        if not outs:
            raise ValueError("Trainer.silhouette_widths: no batches")
        z = torch.cat([o[0] for o in outs], 0)
        metadata = pd.concat([o[1] for o in outs], ignore_index=True)
        return silhouette_widths(z, metadata, **kw)

    @torch.no_grad()
    def cluster_metrics(self, model, batches: Iterable, **kw):
        """`mmvae_amd.clustering.cluster_metrics` of the latent embeddings: z and the metadata gathered exactly as
        `silhouette_widths` gathers them, then per label column a k-means of all cells and its NMI and ARI against the
        labels.  `kw`: label_keys, n_clusters, seed, n_init, max_iter."""
        import pandas as pd

        from .clustering import cluster_metrics
        from .constants import REGISTRY_KEYS as RK

        outs = [p[RK.Z] for p in self.predict(model, batches)]
        if not outs:
            raise ValueError("Trainer.cluster_metrics: no batches")
        z = torch.cat([o[0] for o in outs], 0)
        metadata = pd.concat([o[1] for o in outs], ignore_index=True)
        return cluster_metrics(z, metadata, **kw)

    @torch.no_grad()
    def graph_metrics(self, model, batches: Iterable, **kw):
        """`mmvae_amd.graph_metrics.graph_metrics` of the latent embeddings: z and the metadata gathered exactly as
        `integration_metrics` gathers them, then the graph connectivity of every label column and kBET of the batch
        column (whole graph and per label class) on the exact kNN graph of z.  `kw`: batch_key, label_keys, n_neighbors,
        alpha."""
        import pandas as pd

        from .constants import REGISTRY_KEYS as RK
        from .graph_metrics import graph_metrics

        outs = [p[RK.Z] for p in self.predict(model, batches)]
        if not outs:
            raise ValueError("Trainer.graph_metrics: no batches")
        z = torch.cat([o[0] for o in outs], 0)
        metadata = pd.concat([o[1] for o in outs], ignore_index=True)
        return graph_metrics(z, metadata, **kw)

    @torch.no_grad()
    def pc_regression(self, model, batches: Iterable, **kw):
        """`mmvae_amd.pca.pc_regression` of the latent embeddings: z and the metadata gathered exactly as `graph_metrics`
        gathers them, then the PCA of z and the principal-component regression of every covariate column (categorical
        or numeric) on it.  `kw`: covariates, n_comps."""
        import pandas as pd

        from .constants import REGISTRY_KEYS as RK
        from .pca import pc_regression

        outs = [p[RK.Z] for p in self.predict(model, batches)]
        if not outs:
            raise ValueError("Trainer.pc_regression: no batches")
        z = torch.cat([o[0] for o in outs], 0)
        metadata = pd.concat([o[1] for o in outs], ignore_index=True)
        return pc_regression(z, metadata, **kw)

    @torch.no_grad()
    def correlations(self, model, groups: Iterable, decimals: Optional[int] = 3):
        """The table of get_correlations (runners/run_correlations.py:95-145) as a pandas.DataFrame, one row per group of
        `groups` = (group_id, batch_a, batch_b) with the two batches of different experts
        (`CMMVAEModel.cross_species_correlation`): "group_id", "num_samples" (the cells of batch_a), the eight
        statistic columns, and whichever of RK.FILTER_CATEGORIES batch_a's metadata holds (its first row), sorted by
        group_id as save_correlations does.  Writing the CSV, the pickle and the plot is left to the caller."""
        import pandas as pd

        from .constants import REGISTRY_KEYS as RK

        model.eval()
        model.trainer.set_stage("prediction")
        rows = []
        for group_id, batch_a, batch_b in groups:
            stats = model.cross_species_correlation(batch_a, batch_b, decimals=decimals)
            metadata = batch_a[1]
            cats = {c: metadata[c].iloc[0] for c in RK.FILTER_CATEGORIES if c in metadata.columns}
            rows.append({"group_id": group_id, "num_samples": int(batch_a[0].shape[0]), **stats, **cats})
        table = pd.DataFrame(rows)
        return table.sort_values("group_id").reset_index(drop=True) if rows else table

    @torch.no_grad()
    def meta_discriminators(self, model, batches, **kw) -> list:
        """The meta-discriminators of runners/meta_discriminators.py trained against the frozen model
        (`modules.meta_discriminator.train_meta_discriminators`; `kw`: num_epochs, lr, hidden, labels, include_cis,
        discriminators): one dict per epoch with "meta_disc/md_latent" and "meta_disc/md_<source expert>".  `batches`: a
        re-iterable of `(x, metadata, expert_id)` or a callable returning one epoch's iterable."""
        from .modules.meta_discriminator import train_meta_discriminators

        model.eval()
        model.trainer.set_stage("prediction")
        return train_meta_discriminators(model, batches, **kw)
