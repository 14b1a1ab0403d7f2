"""Meta-discriminators (runners/meta_discriminators.py): small sigmoid MLPs trained AFTER the model, with the model
frozen, to tell from which modality a latent sample or a cross-generated expression matrix came.  Their loss says how
well the modalities mix: ln 2 = indistinguishable.

On the device a discriminator is two GEMMs of libmmvae_hip.so around the fused kernel of libmmvae_disc.so
(ops.disc_tail: everything behind the first layer, the loss and the whole backward in two launches) and one fused Adam
over a flat arena into which every gradient is written directly.  On CPU plumbing the same arithmetic runs in plain
torch (functional.meta_disc_tail in fp64)."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Union

import torch
import torch.nn as nn

from .. import _disc_lib, backend, ops
from .. import functional as HF
from ..constants import REGISTRY_KEYS as RK
from ..optim import HipAdam


class MetaDiscriminator(nn.Module):
    """Linear(in, H1) . Sigmoid . Linear(H1, H2) . Sigmoid . Linear(H2, 1) . Sigmoid  (create_discriminators, :16-55), with
    torch's default nn.Linear initialisation.  The three Linear layers are registered as "0", "2" and "4": the
    state_dict is that of the reference's nn.Sequential, and either side loads the other's.

    Move the module to its device BEFORE the first train_step: that is when its parameters move into the optimiser's
    flat arena (HipAdam, lr as given, no weight decay, no clipping)."""

    def __init__(self, in_features: int, hidden: Sequence[int] = (128, 64), lr: float = 1e-3):
        super().__init__()
        h1, h2 = (int(h) for h in hidden)
        if not (1 <= h1 <= _disc_lib.DISC_MAX_H1 and 1 <= h2 <= _disc_lib.DISC_MAX_H2 and h1 * h2 <= _disc_lib.DISC_MAX_W2):
            raise ValueError(f"MetaDiscriminator: hidden={tuple(hidden)} is outside what the fused kernel takes "
                             f"(H1 <= {_disc_lib.DISC_MAX_H1}, H2 <= {_disc_lib.DISC_MAX_H2}, H1 * H2 <= {_disc_lib.DISC_MAX_W2})")
        self.in_features, self.hidden, self.lr = int(in_features), (h1, h2), float(lr)
        self.add_module("0", nn.Linear(self.in_features, h1))
        self.add_module("2", nn.Linear(h1, h2))
        self.add_module("4", nn.Linear(h2, 1))
        self._opt: Optional[HipAdam] = None
        self._labels: Dict[tuple, torch.Tensor] = {}

    def layers(self):
        m = self._modules
        return m["0"], m["2"], m["4"]

    def as_sequential(self) -> nn.Sequential:
        """The reference's literal nn.Sequential holding copies of these parameters."""
        h1, h2 = self.hidden
        seq = nn.Sequential(nn.Linear(self.in_features, h1), nn.Sigmoid(), nn.Linear(h1, h2), nn.Sigmoid(), nn.Linear(h2, 1),
                            nn.Sigmoid())
        seq.load_state_dict(self.state_dict())
        return seq

    def _check(self, x: torch.Tensor) -> None:
        if x.dim() != 2 or x.shape[1] != self.in_features:
            raise ValueError(f"MetaDiscriminator({self.in_features}): got an input of shape {tuple(x.shape)}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """p [B, 1].  Device tensors: one GEMM and the forward-only kernel (no autograd graph); CPU plumbing: plain torch."""
        self._check(x)
        l1, l2, l3 = self.layers()
        if backend.on_hip(x):
            pre1 = ops.gemm(ops.GEMM_NT, x, l1.weight.data, bias=l1.bias.data)
            p, _, _, _ = ops.disc_tail(pre1, l2.weight.data, l2.bias.data, l3.weight.data, l3.bias.data)
            return p.view(-1, 1)
        return torch.sigmoid(l3(torch.sigmoid(l2(torch.sigmoid(l1(x))))))

    @property
    def optimizer(self) -> HipAdam:
        if self._opt is None:
            self._opt = HipAdam(list(self.parameters()), lr=self.lr, weight_decay=0.0, max_grad_norm=None)
        return self._opt

    def _label(self, y: Union[float, torch.Tensor], B: int, device) -> torch.Tensor:
        if isinstance(y, torch.Tensor):
            y = y.reshape(-1).to(device=device, dtype=torch.float32)
            if y.numel() != B:
                raise ValueError(f"MetaDiscriminator.train_step: {y.numel()} labels for {B} rows")
            return y.contiguous()
        key = (float(y), B, str(device))
        t = self._labels.get(key)
        if t is None:
            t = self._labels[key] = torch.full((B,), float(y), dtype=torch.float32, device=device)
        return t

    @torch.no_grad()
    def train_step(self, x: torch.Tensor, y: Union[float, torch.Tensor]):
        """One Adam step on binary_cross_entropy(self(x), y, reduction="mean") (train_md, :131-163); `x` is a constant (no
        input gradient).  y: one label for every row, or a [B] tensor of labels in [0, 1].  Returns (loss, accuracy) of the
        forward pass AHEAD of the update, as device scalars -- nothing is synchronised."""
        self._check(x)
        l1, l2, l3 = self.layers()
        B = x.shape[0]
        on_hip = backend.on_hip(x)
        opt = self.optimizer
        a = opt.arena
        if a.params[0] is not l1.weight or l1.weight.device != x.device:
            raise RuntimeError("MetaDiscriminator: parameters were replaced or moved after the optimiser was built")
        yv = self._label(y, B, x.device)
        # arena order = parameters() order: 0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias
        dW1, db1, dW2, db2, dW3, db3 = (a.grad_view(i) for i in range(6))
        if on_hip:
            pre1 = ops.gemm(ops.GEMM_NT, x, l1.weight.data, bias=l1.bias.data)
            _, out, dpre1, _ = ops.disc_tail(pre1, l2.weight.data, l2.bias.data, l3.weight.data, l3.bias.data, yv, train=True,
                                             want_p=False, grads=(db1, dW2, db2, dW3, db3))
            ops.gemm(ops.GEMM_TN, dpre1, x, out=dW1)
        else:
            xd = x.double()
            pre1 = xd @ l1.weight.double().T + l1.bias.double()
            _, out, dpre1, g = HF.meta_disc_tail(pre1, l2.weight.data, l2.bias.data, l3.weight.data, l3.bias.data, yv, train=True)
            dW1.copy_(dpre1.T @ xd)
            for dst, src in zip((db1, dW2, db2, dW3, db3), g):
                dst.copy_(src)
            out = out.float()
        opt.note_direct_grads(range(6))
        opt.step()
        return out[0], out[1]


def _latent_width(model) -> int:
    return int(model.module.vae.encoder.mean_encoder.out_features)


def _gene_count(expert) -> int:
    return int(expert.decoder.config.layers[-1])


class MetaDiscriminators(nn.Module):
    """The discriminators of train_md for one model: "latent" over z and one per expert over that expert's generated
    expression, sized from the model and living on its device.

    step(batch) is one iteration of train_md's loop (:117-163) for a batch `(x, metadata, expert_id)` of SOURCE expert s:
    the model cross-generates (eval mode, no_grad; the captured program where the step engine takes the model), "latent"
    takes a step on z with s's label, and for every OTHER expert t the discriminator of t takes a step on xhat_t -- s's
    cells generated through t's decoder -- again with s's label: the reference's policy, generalised to any number of
    experts.  As the reference is written, a species discriminator therefore only ever sees ONE label when there are two
    experts; include_cis=True additionally trains t = s's own discriminator on its cis generation (same label), so that
    every species discriminator sees every label.  Default off: the default reproduces the reference.

    labels: {expert: float}; default 0.0 for the first expert and 1.0 for every other (:131-133)."""

    def __init__(self, model, lr: float = 1e-3, hidden: Sequence[int] = (128, 64), labels: Optional[Dict[str, float]] = None,
                 include_cis: bool = False):
        super().__init__()
        object.__setattr__(self, "model", model)  # (not a submodule: the model is frozen here and saved elsewhere)
        self.experts: List[str] = list(model.module.experts.keys())
        if labels is None:
            labels = {e: (0.0 if i == 0 else 1.0) for i, e in enumerate(self.experts)}
        if set(labels) != set(self.experts):
            raise ValueError(f"MetaDiscriminators: labels for {sorted(labels)}, experts {self.experts}")
        self.labels = {e: float(labels[e]) for e in self.experts}
        self.include_cis = bool(include_cis)
        if "latent" in self.experts:
            raise ValueError('MetaDiscriminators: an expert called "latent" collides with the latent discriminator')
        sizes = {"latent": _latent_width(model)}
        sizes.update({e: _gene_count(model.module.experts[e]) for e in self.experts})
        self.discriminators = nn.ModuleDict({k: MetaDiscriminator(n, hidden, lr=lr) for k, n in sizes.items()})
        self.to(next(model.parameters()).device)
        self.trace: Optional[list] = None  # a list here collects (discriminator, matrix key, label) of every train_step

    def __getitem__(self, name: str) -> MetaDiscriminator:
        return self.discriminators[name]

    def targets_of(self, source: str) -> List[str]:
        return [t for t in self.experts if t != source or self.include_cis]

    @torch.no_grad()
    def step(self, batch, batch_idx: int = 0) -> Dict[str, torch.Tensor]:
        """{"latent": loss, <source expert>: loss} as device scalars: the loss of the latent discriminator, and the loss of
        the target discriminators on this source's generations (their mean when there are several targets)."""
        model = self.model
        source = batch[2]
        if source not in self.labels:
            raise KeyError(f"MetaDiscriminators.step: {source!r} is not an expert of this model ({self.experts})")
        if model.module.training:
            model.eval()
        targets = self.targets_of(source)
        out = model.cross_generate_step(batch, batch_idx, targets=targets)
        label = self.labels[source]
        z = out[RK.Z][0]
        if z.dim() != 2 or z.shape[1] != self.discriminators["latent"].in_features:
            raise ValueError(f"MetaDiscriminators.step: the model returned z of shape {tuple(z.shape)}, the latent "
                             f"discriminator takes {self.discriminators['latent'].in_features} columns")
        losses = {"latent": self._train("latent", RK.Z, z, label)}
        per_target = [self._train(t, f"xhat_{t}", out[f"xhat_{t}"][0], label) for t in targets]
        if per_target:
            losses[source] = per_target[0] if len(per_target) == 1 else torch.stack(per_target).mean()
        return losses

    def _train(self, name: str, key: str, matrix: torch.Tensor, label: float) -> torch.Tensor:
        if self.trace is not None:
            self.trace.append((name, key, label))
        return self.discriminators[name].train_step(matrix, label)[0]


@torch.no_grad()
def train_meta_discriminators(model, batches: Union[Iterable, Callable[[], Iterable]], num_epochs: int = 15, lr: float = 1e-3,
                              hidden: Sequence[int] = (128, 64), labels: Optional[Dict[str, float]] = None,
                              include_cis: bool = False, discriminators: Optional[MetaDiscriminators] = None) -> List[dict]:
    """train_md (:92-167): `num_epochs` passes over `batches` (a re-iterable of `(x, metadata, expert_id)`, or a callable
    that returns the epoch's iterable).  One dict per epoch, the scalars the reference logs: "meta_disc/md_latent" and
    "meta_disc/md_<source expert>" -- the loss of the OTHER experts' discriminators on that source's generations -- each
    the epoch's sum divided by the number of ALL batches of the epoch, as the reference divides.  Losses are added up on
    the device; an epoch costs one transfer.  `discriminators`: train these (e.g. to keep them) instead of new ones."""
    mds = discriminators if discriminators is not None else MetaDiscriminators(model, lr=lr, hidden=hidden, labels=labels,
                                                                               include_cis=include_cis)
    keys = ["latent"] + mds.experts
    device = next(model.parameters()).device
    history = []
    for _ in range(int(num_epochs)):
        acc = torch.zeros(len(keys), dtype=torch.float32, device=device)
        n = 0
        for i, batch in enumerate(batches() if callable(batches) else batches):
            for k, v in mds.step(batch, i).items():
                acc[keys.index(k)] += v
            n += 1
        sums = acc.cpu().tolist()
        history.append({f"meta_disc/md_{k}": (s / n if n else float("nan")) for k, s in zip(keys, sums)})
    return history
