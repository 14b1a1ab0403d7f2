"""Integration metrics on the latent kNN graph: are the modalities mixed, and is the biology kept -- as a number per
cell and per category, from the exact cosine neighbours `umap.knn_graph` computes (libmmvae_mix.so, include/mmvae_mix.h).

    calibrate              per row, the beta whose neighbour weights have the asked perplexity (HIP)
    lisi                   local inverse Simpson's index of code columns: how many categories a neighbourhood mixes (HIP)
    label_transfer         a cell's label voted by its neighbours in the OTHER batches (HIP)
    integration_metrics    the whole call on latent embeddings and their metadata, with a summary table

The definitions are those of include/mmvae_mix.h, in fp64: the neighbours of a row are ranks 1 .. k - 1 of the graph,
their distances shifted by the nearest one's; the calibration is compute_simpson_index of the LISI paper (Korsunsky et
al. 2019; tol 1e-5, at most 50 tries).  Deviations from the published LISI are listed in DESIGN.md: cosine distances of
the exact graph instead of Euclidean ones of an approximate graph, the shift, and k capped at 64.

Device tensors run the HIP kernels, always.  CPU tensors are refused outside `backend.cpu_plumbing()`; inside it every
function is its statement in fp64 (tests/mix_restatement.py restates it independently).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import backend
from ._bind import ptr as _ptr, stream as _stream

TOL = 1e-5
MAX_TRIES = 50
MAX_K = 64
MAX_COLS = 8


# ------------------------------------------------------------------------------------------------------- arguments
def default_perplexity(k: int) -> float:
    """(k - 1) / 3: the LISI convention of three neighbours per unit of perplexity (21 at n_neighbors = 64)."""
    return (k - 1) / 3.0


def _graph(idx: torch.Tensor, dist: torch.Tensor, what: str) -> Tuple[int, int, bool]:
    if idx.dim() != 2 or idx.shape != dist.shape:
        raise ValueError(f"{what}: idx {tuple(idx.shape)} and dist {tuple(dist.shape)} must both be [N, k]")
    N, k = idx.shape
    if not (N >= 1 and 3 <= k <= MAX_K):
        raise ValueError(f"{what}: need N >= 1 and 3 <= k <= {MAX_K} (got N = {N}, k = {k})")
    if idx.device != dist.device:
        raise TypeError(f"{what}: idx is on {idx.device}, dist on {dist.device}")
    hip = backend.on_hip(dist)
    if idx.dtype != torch.int32 or (hip and dist.dtype != torch.float32):
        raise TypeError(f"{what}: expected int32 idx and float32 dist, got {idx.dtype} and {dist.dtype}")
    return N, k, hip


def _perplexity(perplexity: Optional[float], k: int, what: str) -> float:
    u = default_perplexity(k) if perplexity is None else float(perplexity)
    if not (1.0 < u < k - 1):
        raise ValueError(f"{what}: need 1 < perplexity < k - 1 = {k - 1} (got {u})")
    return u


def _check_indices(idx: torch.Tensor, N: int, what: str) -> None:
    """A caller-made graph: the kernels trust idx to lie in [0, N) (one reduction and a host read)."""
    lo, hi = torch.aminmax(idx)
    if int(lo) < 0 or int(hi) >= N:
        raise ValueError(f"{what}: neighbour indices must lie in [0, {N}) (found {int(lo)} .. {int(hi)})")


def _codes(t: torch.Tensor, N: int, like: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.int32:
        raise TypeError(f"{what}: codes must be int32 (negative = unlabelled), got {t.dtype}")
    if t.shape[-1] != N or t.dim() not in (1, 2):
        raise ValueError(f"{what}: codes must be [N] or [n_cols, N] with N = {N}, got {tuple(t.shape)}")
    if t.device != like.device:
        raise TypeError(f"{what}: codes are on {t.device}, the graph on {like.device}")
    return t


# ------------------------------------------------------------------------------------------------ the fp64 statement
def _shifted(dist: torch.Tensor) -> torch.Tensor:
    d = dist.double()
    return d[:, 1:] - d[:, 1:2]


def _weights(beta: torch.Tensor, d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    e = torch.exp(-beta[:, None] * d)
    s = e.sum(1)
    return e / s[:, None], s


def _entropy(beta: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    p, s = _weights(beta, d)
    return torch.log(s) + beta * (d * p).sum(1)


def _calibrate_torch(dist: torch.Tensor, perplexity: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The calibration of include/mmvae_mix.h with torch ops on dist's device, every row moved under a mask."""
    d = _shifted(dist)
    N = d.shape[0]
    log_u = math.log(perplexity)
    inf = float("inf")
    beta = torch.ones(N, dtype=torch.float64, device=d.device)
    lo, hi = torch.full_like(beta, -inf), torch.full_like(beta, inf)
    tries = torch.zeros(N, dtype=torch.int32, device=d.device)
    h = _entropy(beta, d)
    for _ in range(MAX_TRIES):
        move = (h - log_u).abs() > TOL
        if not bool(move.any()):
            break
        up = move & (h > log_u)
        down = move & ~up
        lo, hi = torch.where(up, beta, lo), torch.where(down, beta, hi)
        raised = torch.where(torch.isinf(hi), beta * 2.0, (beta + hi) / 2.0)
        lowered = torch.where(torch.isinf(lo), beta / 2.0, (beta + lo) / 2.0)
        beta = torch.where(up, raised, torch.where(down, lowered, beta))
        tries = tries + move.to(torch.int32)
        h = torch.where(move, _entropy(beta, d), h)
    return beta, tries


def _gathered(codes: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return codes[idx[:, 1:].long()]


def _lisi_torch(idx: torch.Tensor, dist: torch.Tensor, beta: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """[n_cols, N] fp64; the class masses are added rank by rank in ascending order, as the kernel adds them."""
    p, _ = _weights(beta, _shifted(dist))
    out = []
    for col in codes:
        c = _gathered(col, idx)
        labelled = c >= 0
        m = torch.zeros_like(p)
        for l in range(p.shape[1]):
            m = m + torch.where(labelled[:, l:l + 1] & (c == c[:, l:l + 1]), p[:, l:l + 1], torch.zeros_like(p))
        zero = torch.zeros_like(p)
        q = torch.where(labelled, p * m, zero).sum(1)
        t = torch.where(labelled, p, zero).sum(1)
        out.append(torch.where(labelled.any(1), t * t / q, torch.full_like(q, float("nan"))))
    return torch.stack(out)


def _transfer_torch(idx: torch.Tensor, dist: torch.Tensor, beta: torch.Tensor, batch: torch.Tensor,
                    label: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    p, _ = _weights(beta, _shifted(dist))
    bj, lj = _gathered(batch, idx), _gathered(label, idx)
    eligible = (bj >= 0) & (bj != batch[:, None]) & (lj >= 0)
    zero = torch.zeros_like(p)
    pe = torch.where(eligible, p, zero)
    mass = torch.zeros_like(p)
    for l in range(p.shape[1]):
        mass = mass + torch.where(eligible & eligible[:, l:l + 1] & (lj == lj[:, l:l + 1]), pe[:, l:l + 1], zero)
    total = pe.sum(1)
    mass = torch.where(eligible, mass, torch.full_like(mass, -1.0))
    top = mass.max(1).values
    big = torch.iinfo(torch.int32).max
    winner = torch.where(eligible & (mass == top[:, None]), lj, torch.full_like(lj, big)).min(1).values
    voted = eligible.any(1)
    pred = torch.where(voted, winner, torch.full_like(winner, -1)).to(torch.int32)
    conf = torch.where(voted, top / total, torch.zeros_like(top))
    return pred, conf, torch.where(voted, total, torch.zeros_like(total))


# ----------------------------------------------------------------------------------------------------- 1. calibration
def calibrate(idx: torch.Tensor, dist: torch.Tensor, perplexity: Optional[float] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(beta [N] fp64, tries [N] int32) of the graph `knn_graph` returns: per row the beta at which the entropy of the
    neighbour weights P_j ~ exp(-beta d_j) is log(perplexity) within 1e-5, found by at most 50 doubling / halving /
    bisection moves from beta = 1; `tries` counts the moves.  perplexity defaults to (k - 1) / 3; 1 < perplexity < k - 1."""
    N, k, hip = _graph(idx, dist, "calibrate")
    u = _perplexity(perplexity, k, "calibrate")
    if not hip:
        return _calibrate_torch(dist, u)
    from . import _mix_lib

    idx, dist = idx.contiguous(), dist.contiguous()
    beta = torch.empty(N, dtype=torch.float64, device=dist.device)
    tries = torch.empty(N, dtype=torch.int32, device=dist.device)
    _mix_lib.check(_mix_lib.load_mix().mmvae_mix_calibrate_f32(N, k, _ptr(idx), _ptr(dist), u, _ptr(beta), _ptr(tries),
                                                               _stream()), "mmvae_mix_calibrate_f32")
    return beta, tries


def _beta(idx, dist, perplexity, beta, N, what) -> torch.Tensor:
    if beta is None:
        return calibrate(idx, dist, perplexity)[0]
    if perplexity is not None:
        raise ValueError(f"{what}: give perplexity or beta, not both")
    if beta.shape != (N,) or beta.dtype != torch.float64 or beta.device != dist.device:
        raise TypeError(f"{what}: beta must be float64 [N] on the graph's device, as calibrate returns it")
    return beta.contiguous()


# ------------------------------------------------------------------------------------------------------------ 2. LISI
def lisi(idx: torch.Tensor, dist: torch.Tensor, codes: torch.Tensor, perplexity: Optional[float] = None,
         beta: Optional[torch.Tensor] = None, *, _trusted: bool = False) -> torch.Tensor:
    """Local inverse Simpson's index of `codes` ([N] or [n_cols, N] int32, negative = unlabelled) in every row's
    neighbourhood, in the shape of `codes`: 1 where all labelled neighbours share one class, up to the number of classes
    where they mix evenly, NaN where no neighbour is labelled.  The row's own code is not used.  `beta` is `calibrate`'s
    (computed from `perplexity` when absent).  Up to eight columns share one launch."""
    N, k, hip = _graph(idx, dist, "lisi")
    cols = _codes(codes, N, dist, "lisi")
    beta = _beta(idx, dist, perplexity, beta, N, "lisi")
    if not _trusted:
        _check_indices(idx, N, "lisi")
    flat = cols.reshape(-1, N)
    if not hip:
        return _lisi_torch(idx, dist, beta, flat).reshape(codes.shape)
    from . import _mix_lib

    lib = _mix_lib.load_mix()
    idx, dist = idx.contiguous(), dist.contiguous()
    if flat.stride(-1) != 1 or (flat.shape[0] > 1 and flat.stride(0) < N):
        flat = flat.contiguous()
    ldc = flat.stride(0) if flat.shape[0] > 1 else N
    out = torch.empty((flat.shape[0], N), dtype=torch.float32, device=dist.device)
    for c0 in range(0, flat.shape[0], MAX_COLS):
        n_cols = min(MAX_COLS, flat.shape[0] - c0)
        _mix_lib.check(lib.mmvae_mix_lisi_f32(N, k, _ptr(idx), _ptr(dist), _ptr(beta), n_cols, _ptr(flat[c0]), ldc,
                                              _ptr(out[c0]), N, _stream()), "mmvae_mix_lisi_f32")
    return out.reshape(codes.shape)


# -------------------------------------------------------------------------------------------------- 3. label transfer
def label_transfer(idx: torch.Tensor, dist: torch.Tensor, batch: torch.Tensor, label: torch.Tensor,
                   perplexity: Optional[float] = None, beta: Optional[torch.Tensor] = None, *, _trusted: bool = False
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pred [N] int32, conf [N], cross [N]): every cell's label as voted by its neighbours in the other batches.  A
    neighbour votes when it is in a batch other than the cell's and carries a label (codes >= 0); cross is the weight of
    the voters (0: the neighbourhood holds no other batch), pred the label with the largest voting weight (ties: the
    smallest code; -1 without voters) and conf that weight's share of cross.  The cell's own label is not used."""
    N, k, hip = _graph(idx, dist, "label_transfer")
    for name, t in (("batch", batch), ("label", label)):
        if _codes(t, N, dist, "label_transfer").dim() != 1:
            raise ValueError(f"label_transfer: {name} must be [N]")
    beta = _beta(idx, dist, perplexity, beta, N, "label_transfer")
    if not _trusted:
        _check_indices(idx, N, "label_transfer")
    if not hip:
        return _transfer_torch(idx, dist, beta, batch, label)
    from . import _mix_lib

    idx, dist, batch, label = idx.contiguous(), dist.contiguous(), batch.contiguous(), label.contiguous()
    pred = torch.empty(N, dtype=torch.int32, device=dist.device)
    conf = torch.empty(N, dtype=torch.float32, device=dist.device)
    cross = torch.empty_like(conf)
    _mix_lib.check(_mix_lib.load_mix().mmvae_mix_transfer_f32(N, k, _ptr(idx), _ptr(dist), _ptr(beta), _ptr(batch),
                                                              _ptr(label), _ptr(pred), _ptr(conf), _ptr(cross), _stream()),
                   "mmvae_mix_transfer_f32")
    return pred, conf, cross


# ------------------------------------------------------------------------------------------------------ 4. whole call
@dataclass
class IntegrationMetrics:
    """What `integration_metrics` returns.  The per-cell tensors stay on the embeddings' device; the tables are pandas
    frames on the host."""
    idx: torch.Tensor                 # [N, k] int32: the kNN graph the metrics were read from
    dist: torch.Tensor                # [N, k]
    beta: torch.Tensor                # [N] fp64
    tries: torch.Tensor               # [N] int32
    columns: Tuple[str, ...]          # the batch column first, then the label columns
    codes: torch.Tensor               # [n_columns, N] int32, -1 = missing
    categories: Dict[str, object]     # column -> the pandas Index its codes point into
    lisi: torch.Tensor                # [n_columns, N]
    summary: object                   # DataFrame, one row per column
    pred: Dict[str, torch.Tensor] = field(default_factory=dict)    # label column -> [N] int32
    conf: Dict[str, torch.Tensor] = field(default_factory=dict)
    cross: Dict[str, torch.Tensor] = field(default_factory=dict)
    confusion: Dict[str, object] = field(default_factory=dict)     # label column -> DataFrame (rows true, columns predicted)
    transfer_summary: Optional[object] = None                      # DataFrame, one row per (label column, batch)


SUMMARY_COLUMNS = ("column", "role", "n_classes", "n_cells", "mean_lisi", "median_lisi", "scaled_lisi")
TRANSFER_COLUMNS = ("label", "batch", "n_cells", "n_scored", "accuracy", "mean_cross", "share_without_neighbour")


def factorize(column) -> Tuple[torch.Tensor, object]:
    """(codes [N] int32 on the host, categories) of a metadata column through pandas.factorize: sorted categories where
    the values can be sorted, NaN -> -1."""
    import numpy as np
    import pandas as pd

    try:
        codes, uniques = pd.factorize(column, sort=True)
    except TypeError:  # values of several types: the order of first appearance
        codes, uniques = pd.factorize(column, sort=False)
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)), uniques


def _nan_stats(values: torch.Tensor) -> Tuple[int, float, float]:
    v = values[~torch.isnan(values)].double()
    if v.numel() == 0:
        return 0, float("nan"), float("nan")
    return v.numel(), float(v.mean()), float(v.median())


def summarise_lisi(lisi_rows: torch.Tensor, columns: Sequence[str], roles: Sequence[str], n_classes: Sequence[int]):
    """One row per column: the number of classes, the cells with a defined LISI, their mean and median (fp64 on the
    tensors' device) and the scaled value (median - 1) / (classes - 1): 0 = one class per neighbourhood, 1 = all of them
    evenly.  For a batch column 1 is the goal, for a label column 0."""
    import pandas as pd

    rows = []
    for name, role, classes, values in zip(columns, roles, n_classes, lisi_rows):
        n, mean, median = _nan_stats(values)
        scaled = (median - 1.0) / (classes - 1.0) if classes > 1 else float("nan")
        rows.append((name, role, int(classes), n, mean, median, scaled))
    return pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS))


def summarise_transfer(name: str, batch: torch.Tensor, label: torch.Tensor, pred: torch.Tensor, cross: torch.Tensor,
                       batch_names: Sequence, label_names: Sequence):
    """(rows of the transfer table, confusion DataFrame) of one label column.  Per batch (cells outside every batch are
    left out) and once over "all" cells: the accuracy over the cells that have a label and a prediction, the mean cross
    weight and the share of cells without an eligible neighbour.  Counted with fp64 bincounts on the tensors' device."""
    import pandas as pd

    B, L = len(batch_names), len(label_names)
    f64 = torch.float64
    in_batch = batch >= 0
    scored = in_batch & (label >= 0) & (pred >= 0)
    bl = batch.long()

    def per_batch(mask, weights=None):
        w = None if weights is None else weights[mask].to(f64)
        return torch.bincount(bl[mask], weights=w, minlength=B).to(f64)

    cells = per_batch(in_batch)
    n_scored = per_batch(scored)
    right = per_batch(scored, (pred == label))
    cross_sum = per_batch(in_batch, cross)
    lonely = per_batch(in_batch & (pred < 0))
    table = torch.stack([cells, n_scored, right, cross_sum, lonely]).cpu()
    everyone = (label >= 0) & (pred >= 0)
    total = torch.stack([torch.tensor(float(batch.numel()), dtype=f64), everyone.sum().to(f64).cpu(),
                         (everyone & (pred == label)).sum().to(f64).cpu(), cross.to(f64).sum().cpu(),
                         (pred < 0).sum().to(f64).cpu()])

    def row(who, t):
        n, s, r, c, z = (float(v) for v in t)
        nan = float("nan")
        return (name, who, int(n), int(s), r / s if s else nan, c / n if n else nan, z / n if n else nan)

    rows = [row(batch_names[b], table[:, b]) for b in range(B)] + [row("all", total)]
    counts = torch.bincount(label.long()[everyone] * L + pred.long()[everyone], minlength=L * L).view(L, L).cpu().numpy()
    confusion = pd.DataFrame(counts, index=pd.Index(list(label_names), name="true"),
                             columns=pd.Index(list(label_names), name="predicted"))
    return rows, confusion


def integration_metrics(z: torch.Tensor, metadata, batch_key: str = "species", label_keys: Sequence[str] = ("cell_type",),
                        n_neighbors: int = 64, perplexity: Optional[float] = None, transfer: bool = True
                        ) -> IntegrationMetrics:
    """LISI and label transfer of latent embeddings z [N, D] with one metadata row per cell.

    `umap.knn_graph(z, n_neighbors)`, one calibration, one LISI launch over the batch column and every label column, and
    (transfer=True) one label transfer per label column across the batches.  Codes come from pandas.factorize, NaN = -1.
    The summary has one row per column (SUMMARY_COLUMNS); transfer_summary one row per label column and batch plus an
    "all" row (TRANSFER_COLUMNS); confusion[label column] counts true against predicted labels."""
    import pandas as pd

    from .umap import knn_graph

    if isinstance(label_keys, str):
        label_keys = (label_keys,)
    columns = (batch_key,) + tuple(label_keys)
    missing = [c for c in columns if c not in metadata.columns]
    if missing:
        raise KeyError(f"integration_metrics: metadata has no column {missing} (it has {list(metadata.columns)})")
    if len(metadata) != z.shape[0]:
        raise ValueError(f"integration_metrics: {z.shape[0]} embeddings but {len(metadata)} metadata rows")
    idx, dist = knn_graph(z, n_neighbors)
    factored = [factorize(metadata[c]) for c in columns]
    categories = {c: u for c, (_, u) in zip(columns, factored)}
    codes = torch.stack([f[0] for f in factored]).to(z.device)
    beta, tries = calibrate(idx, dist, perplexity)
    values = lisi(idx, dist, codes, beta=beta, _trusted=True)
    roles = ["batch"] + ["label"] * len(label_keys)
    summary = summarise_lisi(values, columns, roles, [len(categories[c]) for c in columns])
    out = IntegrationMetrics(idx, dist, beta, tries, columns, codes, categories, values, summary)
    if transfer:
        rows = []
        for n, key in enumerate(label_keys, start=1):
            pred, conf, cross = label_transfer(idx, dist, codes[0], codes[n], beta=beta, _trusted=True)
            out.pred[key], out.conf[key], out.cross[key] = pred, conf, cross
            r, out.confusion[key] = summarise_transfer(key, codes[0], codes[n], pred, cross, list(categories[batch_key]),
                                                       list(categories[key]))
            rows += r
        out.transfer_summary = pd.DataFrame(rows, columns=list(TRANSFER_COLUMNS))
    return out


def _display(v):
    return v.decode() if isinstance(v, bytes) else v


def write_tables(result: IntegrationMetrics, save_dir: str, key: str) -> list:
    """`save_dir`/integration_metrics.{key}.csv (the summary) and, where a transfer was made,
    integration_metrics.{key}.transfer.csv and one integration_metrics.{key}.confusion.{label column}.csv; the paths."""
    import os

    os.makedirs(save_dir, exist_ok=True)
    paths = [os.path.join(save_dir, f"integration_metrics.{key}.csv")]
    result.summary.to_csv(paths[0], index=False)
    if result.transfer_summary is not None:
        paths.append(os.path.join(save_dir, f"integration_metrics.{key}.transfer.csv"))
        result.transfer_summary.assign(batch=result.transfer_summary["batch"].map(_display)).to_csv(paths[-1], index=False)
        for name, table in result.confusion.items():
            paths.append(os.path.join(save_dir, f"integration_metrics.{key}.confusion.{name}.csv"))
            table.rename(index=_display, columns=_display).to_csv(paths[-1])
    return paths


def metrics_from_predictions(directory: str, keys: Sequence[str], batch_key: str = "species",
                             label_keys: Sequence[str] = ("cell_type",), save_dir: Optional[str] = None, **kw) -> list:
    """`integration_metrics` of stored predictions, in the two input forms of `plots.generate_umap`: a directory holding
    `{key}_embeddings.npz` with `{key}_metadata.pkl`, or a predictions.h5 read through `predictions.load_from_hdf5`.
    Writes the tables of `write_tables` into `save_dir` (default: the directory, or the file's) and returns their paths."""
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
        result = integration_metrics(_as_points(X), metadata, batch_key, label_keys, **kw)
        paths += write_tables(result, out_dir, key)
    return paths
