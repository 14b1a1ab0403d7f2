"""Silhouette widths of latent embeddings: the global companion of the kNN-graph metrics of `mmvae_amd.mixing` -- per
cell, the mean distance to its own class against the nearest other class, over all cells (libmmvae_sil.so,
include/mmvae_sil.h), and the two averages every integration benchmark reports (scIB, Luecken et al. 2022).

    sort_runs              the order that makes classes contiguous inside groups, and its run tables
    silhouette_samples     a, b, s and the nearest other class of every cell (HIP)
    asw_label              mean silhouette of the labels
    asw_batch              mean of 1 - |s| of the batches inside every label, averaged over the labels
    silhouette_widths      the whole call on latent embeddings and their metadata, with summary tables

The definitions are those of include/mmvae_sil.h.  Device tensors run the HIP kernels, always.  CPU tensors are refused
outside `backend.cpu_plumbing()`; inside it every function is its statement in fp64 (tests/sil_restatement.py restates it
independently).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import backend
from ._bind import ptr as _ptr, stream as _stream

MAX_D = 512
METRICS = {"euclidean": 0, "cosine": 1}


class SilhouetteRows(NamedTuple):
    """Per cell, in the caller's row order: a the mean distance to the own class, b to the nearest other class of the
    group, s the silhouette, nearest that class's code (-1: none).  Cells without a class or group: NaN and -1."""
    a: torch.Tensor
    b: torch.Tensor
    s: torch.Tensor
    nearest: torch.Tensor


# ---------------------------------------------------------------------------------------------------------- the runs
def _codes(t: torch.Tensor, N: int, like: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: codes must be int32 or int64 (negative = unlabelled), got {t.dtype}")
    if t.shape != (N,):
        raise ValueError(f"{what}: codes must be [N] with N = {N}, got {tuple(t.shape)}")
    if t.device != like.device:
        raise TypeError(f"{what}: codes are on {t.device}, the rows on {like.device}")
    return t


def sort_runs(cls: torch.Tensor, group: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(order [n] int64, run_ptr [R + 1] int32, run_group [R] int32, run_class [R] int32) of class codes [N] and, where
    given, group codes [N].  Cells with a negative class or group code are dropped; the rest are sorted stably by
    (group, class), so that `order` lists, run after run, the cells of one class of one group in their original order.
    Without `group` all cells form group 0.  Torch ops on the codes' device."""
    if cls.dim() != 1 or (group is not None and group.shape != cls.shape):
        raise ValueError("sort_runs: cls and group must be [N]")
    keep = cls >= 0
    if group is not None:
        keep = keep & (group >= 0)
    kept = torch.nonzero(keep).flatten()
    c = cls[kept].long()
    g = group[kept].long() if group is not None else torch.zeros_like(c)
    by_class = torch.argsort(c, stable=True)
    by_group = torch.argsort(g[by_class], stable=True)
    inner = by_class[by_group]
    order, c, g = kept[inner], c[inner], g[inner]
    n = order.numel()
    i32 = dict(dtype=torch.int32, device=cls.device)
    if n == 0:
        empty = torch.zeros(0, **i32)
        return order, torch.zeros(1, **i32), empty, empty.clone()
    change = (c[1:] != c[:-1]) | (g[1:] != g[:-1])
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=cls.device), torch.nonzero(change).flatten() + 1])
    run_ptr = torch.cat([starts, torch.full((1,), n, dtype=torch.int64, device=cls.device)]).to(torch.int32)
    return order, run_ptr, g[starts].to(torch.int32), c[starts].to(torch.int32)


# ------------------------------------------------------------------------------------------------ the fp64 statement
def _rows_torch(x: torch.Tensor, metric: int, run_ptr: torch.Tensor, run_group: torch.Tensor):
    """(a, b, s fp64, nearest int32) of sorted rows, as include/mmvae_sil.h defines them, with torch ops in fp64."""
    x = x.double()
    n, R = x.shape[0], run_group.numel()
    counts = (run_ptr[1:] - run_ptr[:-1]).long()
    run_of = torch.repeat_interleave(torch.arange(R, device=x.device), counts)
    onehot = torch.zeros((n, R), dtype=torch.float64, device=x.device)
    onehot[torch.arange(n, device=x.device), run_of] = 1.0
    if metric == 1:
        norm = x.pow(2).sum(1).sqrt()
        x = x * torch.where(norm > 0, 1.0 / norm, torch.zeros_like(norm))[:, None]
    sums = torch.empty((n, R), dtype=torch.float64, device=x.device)
    for i0 in range(0, n, 1024):
        rows = x[i0:i0 + 1024]
        if metric == 1:
            d = (1.0 - rows @ x.T).clamp_min(0.0)
        else:
            d = torch.cdist(rows, x, compute_mode="donot_use_mm_for_euclid_dist")
        d[torch.arange(rows.shape[0]), torch.arange(i0, i0 + rows.shape[0])] = 0.0
        sums[i0:i0 + 1024] = d @ onehot
    cnt = counts.double()
    own = onehot.bool()
    n_own = cnt[run_of]
    a = torch.where(n_own > 1, sums[own] / (n_own - 1).clamp_min(1.0), torch.zeros_like(n_own))
    other = (run_group[run_of].long()[:, None] == run_group.long()[None, :]) & ~own
    means = torch.where(other, sums / cnt[None, :], torch.full_like(sums, float("inf")))
    b, nearest = means.min(1)  # (the first minimum: ties go to the smaller run)
    alone = ~other.any(1)
    nan = torch.full_like(b, float("nan"))
    b = torch.where(alone, nan, b)
    top = torch.maximum(a, b)
    s = torch.where((n_own == 1) | (top == 0), torch.zeros_like(b), (b - a) / top)
    s = torch.where(alone, nan, s)
    nearest = torch.where(alone, torch.full_like(nearest, -1), nearest).to(torch.int32)
    return a, b, s, nearest


# ------------------------------------------------------------------------------------------------------ 1. per cell
def silhouette_rows(x: torch.Tensor, run_ptr: torch.Tensor, run_group: torch.Tensor, metric: str = "euclidean"
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(a, b, s [n], nearest [n] int32 run indices) of rows already sorted into runs -- the entry of include/mmvae_sil.h as
    it stands: no centring, `nearest` a run index.  x [n, D] float32 with unit column stride (any row stride >= D).  The
    seam under `silhouette_samples`, and what tools/bench_silhouette.py times.  On the device a, b, s are fp32, as the
    library stores them; on CPU plumbing they are the fp64 statement, unrounded."""
    if metric not in METRICS:
        raise ValueError(f"silhouette: metric must be one of {sorted(METRICS)}, got {metric!r}")
    if x.dim() != 2 or not (x.shape[0] >= 1 and 1 <= x.shape[1] <= MAX_D):
        raise ValueError(f"silhouette: x must be [N, D] with N >= 1 and 1 <= D <= {MAX_D}, got {tuple(x.shape)}")
    n, D = x.shape
    R = run_group.numel()
    if run_ptr.shape != (R + 1,) or not 1 <= R <= n or run_ptr.dtype != torch.int32 or run_group.dtype != torch.int32:
        raise ValueError("silhouette: run_ptr [R + 1] and run_group [R] must be int32 with 1 <= R <= N")
    if run_ptr.device != x.device or run_group.device != x.device:
        raise TypeError("silhouette: the run tables must be on the rows' device")
    if not backend.on_hip(x):
        return _rows_torch(x, METRICS[metric], run_ptr, run_group)
    if x.dtype != torch.float32:
        raise TypeError(f"silhouette: expected float32 rows, got {x.dtype}")
    from . import _sil_lib

    lib = _sil_lib.load_sil()
    if x.stride(1) != 1 or (n > 1 and x.stride(0) < D):
        x = x.contiguous()
    ldx = x.stride(0) if n > 1 else D
    run_ptr, run_group = run_ptr.contiguous(), run_group.contiguous()
    f32 = dict(dtype=torch.float32, device=x.device)
    a, b, s = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32)
    nearest = torch.empty(n, dtype=torch.int32, device=x.device)
    nbytes = lib.mmvae_sil_rows_workspace_bytes(n, D)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _sil_lib.check(lib.mmvae_sil_rows_f32(n, D, _ptr(x), ldx, METRICS[metric], R, _ptr(run_ptr), _ptr(run_group), _ptr(a),
                                          _ptr(b), _ptr(nearest), _ptr(s), _ptr(workspace), nbytes, _stream()),
                   "mmvae_sil_rows_f32")
    return a, b, s, nearest


def silhouette_samples(x: torch.Tensor, cls: torch.Tensor, group: Optional[torch.Tensor] = None,
                       metric: str = "euclidean") -> SilhouetteRows:
    """The silhouette of every row of x [N, D] for the class codes `cls` [N], taken inside the groups `group` [N] where
    given (a cell is compared with the cells of its own group only).  Results are in the caller's row order on x's
    device; cells with a negative class or group code are left out of every mean and get NaN (nearest -1).  `nearest` is
    the class CODE of the nearest other class.  For the Euclidean metric the kept rows are centred on their fp64 column
    mean before the launch: a translation changes no distance and shrinks the cancellation of the Gram form."""
    if x.dim() != 2:
        raise ValueError(f"silhouette_samples: x must be [N, D], got {tuple(x.shape)}")
    N = x.shape[0]
    _codes(cls, N, x, "silhouette_samples")
    if group is not None:
        _codes(group, N, x, "silhouette_samples")
    hip = backend.on_hip(x)
    order, run_ptr, run_group, run_class = sort_runs(cls, group)
    dtype = torch.float32 if hip else torch.float64
    nan = float("nan")
    out = [torch.full((N,), nan, dtype=dtype, device=x.device) for _ in range(3)]
    nearest = torch.full((N,), -1, dtype=torch.int32, device=x.device)
    if order.numel() == 0:
        return SilhouetteRows(*out, nearest)
    if hip and x.dtype != torch.float32:
        raise TypeError(f"silhouette_samples: expected float32 rows, got {x.dtype}")
    rows = x[order]
    if metric == "euclidean" and hip:
        rows64 = rows.double()
        rows = (rows64 - rows64.mean(0, keepdim=True)).float()
    a, b, s, near = silhouette_rows(rows, run_ptr, run_group, metric)
    for full, part in zip(out, (a, b, s)):
        full[order] = part
    nearest[order] = torch.where(near >= 0, run_class[near.clamp_min(0).long()], near)
    return SilhouetteRows(*out, nearest)


# ------------------------------------------------------------------------------------------------------- 2. averages
def asw_label(s: torch.Tensor, scaled: bool = False) -> float:
    """Mean of the defined silhouettes (NaN with none); scaled=True gives (mean + 1) / 2, scIB's form in [0, 1]."""
    v = s[~torch.isnan(s)].double()
    mean = float(v.mean()) if v.numel() else float("nan")
    return (mean + 1.0) / 2.0 if scaled else mean


def _batch_means(s: torch.Tensor, label: torch.Tensor, n_labels: int, batch: Optional[torch.Tensor] = None):
    """Per label code 0 .. n_labels - 1: (mean of 1 - |s| over its cells with a defined s -- NaN for a skipped label --,
    the number of those cells) as fp64 tensors on s's device."""
    ok = ~torch.isnan(s) & (label >= 0)
    ll = label.long()
    w = 1.0 - s.double().abs()
    total = torch.bincount(ll[ok], weights=w[ok], minlength=n_labels)
    n = torch.bincount(ll[ok], minlength=n_labels).double()
    skip = n == 0
    if batch is not None:  # scIB: a label whose every batch is a single cell has no batch silhouette either
        both = ok & (batch >= 0)
        pairs = torch.unique(torch.stack([ll[both], batch.long()[both]]), dim=1)
        n_batches = torch.bincount(pairs[0], minlength=n_labels).double()
        skip = skip | (n_batches == torch.bincount(ll[both], minlength=n_labels).double())
    mean = torch.where(skip, torch.full_like(n, float("nan")), total.double() / n.clamp_min(1.0))
    return mean, torch.where(skip, torch.zeros_like(n), n)


def asw_batch(s: torch.Tensor, label: torch.Tensor, batch: Optional[torch.Tensor] = None) -> float:
    """scIB's batch ASW of the silhouettes `s` of the batches taken inside every label (`silhouette_samples(x, batch,
    group=label)`): per label the mean of 1 - |s| over its cells with a defined s, then the mean over the labels.  A label
    with a single batch has no defined s and is skipped; with `batch` given, so is a label whose every batch is a single
    cell (s = 0 by convention there, which scIB leaves out).  1 = the batches of every label are mixed."""
    if label.numel() == 0 or int(label.max()) < 0:
        return float("nan")
    mean, _ = _batch_means(s, label, int(label.max()) + 1, batch)
    mean = mean[~torch.isnan(mean)]
    return float(mean.mean()) if mean.numel() else float("nan")


# ------------------------------------------------------------------------------------------------------ 3. whole call
@dataclass
class SilhouetteWidths:
    """What `silhouette_widths` returns.  The per-cell tensors stay on the embeddings' device; the tables are pandas
    frames on the host."""
    columns: Tuple[str, ...]                  # the batch column first, then the label columns
    codes: torch.Tensor                       # [n_columns, N] int32, -1 = missing
    categories: Dict[str, object]             # column -> the pandas Index its codes point into
    metric: str
    summary: object                           # DataFrame, one row per (label column, role)
    label_rows: Dict[str, SilhouetteRows] = field(default_factory=dict)   # label column -> silhouette of the labels
    batch_rows: Dict[str, SilhouetteRows] = field(default_factory=dict)   # label column -> of the batches inside it
    per_label: Dict[str, object] = field(default_factory=dict)            # label column -> DataFrame, one row per class


SUMMARY_COLUMNS = ("column", "role", "n_classes", "n_cells", "asw", "scaled")
PER_LABEL_COLUMNS = ("n_cells", "n_batches", "label_asw", "batch_asw")


def silhouette_widths(z: torch.Tensor, metadata, batch_key: str = "species", label_keys: Sequence[str] = ("cell_type",),
                      metric: str = "euclidean") -> SilhouetteWidths:
    """Label and batch ASW of latent embeddings z [N, D] with one metadata row per cell.

    Codes come from `mixing.factorize` (NaN = -1).  Per label column two launches: class = label over a single group (the
    label silhouette), and class = batch with group = label (the batch silhouette inside every label).  The summary
    (SUMMARY_COLUMNS) has two rows per label column: role "label" -- the classes, the cells with a defined s, their mean
    and (mean + 1) / 2 -- and role "batch" -- the labels that count, their cells with a defined s, `asw_batch` and the
    same value again (it lies in [0, 1] already).  per_label[column] (PER_LABEL_COLUMNS) has one row per class."""
    import pandas as pd

    from .mixing import factorize

    if isinstance(label_keys, str):
        label_keys = (label_keys,)
    columns = (batch_key,) + tuple(label_keys)
    missing = [c for c in columns if c not in metadata.columns]
    if missing:
        raise KeyError(f"silhouette_widths: metadata has no column {missing} (it has {list(metadata.columns)})")
    if len(metadata) != z.shape[0]:
        raise ValueError(f"silhouette_widths: {z.shape[0]} embeddings but {len(metadata)} metadata rows")
    backend.on_hip(z)
    factored = [factorize(metadata[c]) for c in columns]
    categories = {c: u for c, (_, u) in zip(columns, factored)}
    codes = torch.stack([f[0] for f in factored]).to(z.device)
    out = SilhouetteWidths(columns, codes, categories, metric, None)
    batch = codes[0]
    rows = []
    for n, key in enumerate(label_keys, start=1):
        label, L = codes[n], len(categories[key])
        of_label = silhouette_samples(z, label, None, metric)
        of_batch = silhouette_samples(z, batch, label, metric)
        out.label_rows[key], out.batch_rows[key] = of_label, of_batch
        mean = asw_label(of_label.s)
        rows.append((key, "label", L, int((~torch.isnan(of_label.s)).sum()), mean, (mean + 1.0) / 2.0))
        per_batch, counted = _batch_means(of_batch.s, label, L, batch)
        used = ~torch.isnan(per_batch)
        value = float(per_batch[used].mean()) if bool(used.any()) else float("nan")
        rows.append((key, "batch", int(used.sum()), int(counted.sum()), value, value))
        has = label >= 0
        ll = label.long()[has]
        cells = torch.bincount(ll, minlength=L)
        inside = has & (batch >= 0)
        pairs = torch.unique(torch.stack([label.long()[inside], batch.long()[inside]]), dim=1)
        n_batches = torch.bincount(pairs[0], minlength=L)
        defined = has & ~torch.isnan(of_label.s)
        total = torch.bincount(label.long()[defined], weights=of_label.s.double()[defined], minlength=L)
        n_defined = torch.bincount(label.long()[defined], minlength=L).double()
        label_mean = torch.where(n_defined > 0, total.double() / n_defined.clamp_min(1.0),
                                 torch.full_like(n_defined, float("nan")))
        out.per_label[key] = pd.DataFrame(
            {"n_cells": cells.cpu().numpy(), "n_batches": n_batches.cpu().numpy(), "label_asw": label_mean.cpu().numpy(),
             "batch_asw": per_batch.cpu().numpy()}, index=pd.Index(list(categories[key]), name=key))
    out.summary = pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS))
    return out


def _display(v):
    return v.decode() if isinstance(v, bytes) else v


def write_tables(result: SilhouetteWidths, save_dir: str, key: str) -> list:
    """`save_dir`/silhouette.{key}.csv (the summary) and one silhouette.{key}.{label column}.csv per label column (its
    per-class table); the paths."""
    import os

    os.makedirs(save_dir, exist_ok=True)
    paths = [os.path.join(save_dir, f"silhouette.{key}.csv")]
    result.summary.to_csv(paths[0], index=False)
    for name, table in result.per_label.items():
        paths.append(os.path.join(save_dir, f"silhouette.{key}.{name}.csv"))
        table.rename(index=_display).to_csv(paths[-1])
    return paths


def widths_from_predictions(directory: str, keys: Sequence[str], batch_key: str = "species",
                            label_keys: Sequence[str] = ("cell_type",), save_dir: Optional[str] = None, **kw) -> list:
    """`silhouette_widths` of stored predictions, in the two input forms of `mixing.metrics_from_predictions`: a directory
    holding `{key}_embeddings.npz` with `{key}_metadata.pkl`, or a predictions.h5.  Writes the tables of `write_tables`
    into `save_dir` (default: the directory, or the file's) and returns their paths."""
    import os

    from .plots import _as_points, _load_pair

    paths = []
    for key in keys:
        if directory.endswith(".h5"):
            from . import predictions as P

            if not os.path.exists(directory):
                raise FileNotFoundError(directory)
            X, metadata, _ = P.load_from_hdf5(directory, key)
            if X is None or metadata is None:
                raise KeyError(f"{directory}: group {key!r} holds no embeddings with metadata")
            out_dir = save_dir or os.path.dirname(directory) or "."
        else:
            X, metadata = _load_pair(os.path.join(directory, f"{key}_embeddings.npz"),
                                     os.path.join(directory, f"{key}_metadata.pkl"))
            out_dir = save_dir or directory
        result = silhouette_widths(_as_points(X), metadata, batch_key, label_keys, **kw)
        paths += write_tables(result, out_dir, key)
    return paths
