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


class Trainer:
    def __init__(self, max_epochs: int = 10, max_steps: int = -1, limit_train_batches: Optional[int] = None,
                 limit_val_batches: Optional[int] = None, check_val_every_n_epoch: int = 1,
                 num_sanity_val_steps: int = 0, **unused):
        self.max_epochs = max_epochs
        self.max_steps = max_steps
        self.limit_train_batches = limit_train_batches
        self.limit_val_batches = limit_val_batches
        self.check_val_every_n_epoch = check_val_every_n_epoch
        self.num_sanity_val_steps = num_sanity_val_steps
        self.global_step = 0
        self.history: List[dict] = []

    @classmethod
    def from_yaml(cls, path: str) -> "Trainer":
        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
        keys = ("max_epochs", "max_steps", "limit_train_batches", "limit_val_batches", "check_val_every_n_epoch",
                "num_sanity_val_steps")
        return cls(**{k: cfg[k] for k in keys if cfg.get(k) is not None})

    def _snapshot(self, model) -> dict:
        return {k: (float(v.detach()) if torch.is_tensor(v) else v) for k, v in model.logged.items()}

    def fit(self, model, train_batches: Iterable, val_batches: Optional[Iterable] = None):
        model.optimizers()
        stub = model.trainer
        for epoch in range(self.max_epochs):
            model.train()
            stub.set_stage("training")
            for i, batch in enumerate(Lookahead(train_batches, model) if hasattr(model, "hint_next_batch") else train_batches):
                if self.limit_train_batches is not None and i >= self.limit_train_batches:
                    break
                model.training_step(batch, i)
                self.global_step += 1
                stub.global_step = self.global_step
                if 0 < self.max_steps <= self.global_step:
                    break
            self.history.append({"epoch": epoch, "stage": "training", **self._snapshot(model)})
            if val_batches is not None and (epoch + 1) % self.check_val_every_n_epoch == 0:
                self.validate(model, val_batches)
            if 0 < self.max_steps <= self.global_step:
                break
        return self.history

    @torch.no_grad()
    def validate(self, model, batches: Iterable):
        model.eval()
        model.trainer.set_stage("validation")
        for i, batch in enumerate(batches):
            if self.limit_val_batches is not None and i >= self.limit_val_batches:
                break
            model.validation_step(batch, i)
        self.history.append({"stage": "validation", **self._snapshot(model)})

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
