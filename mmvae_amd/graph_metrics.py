"""Graph connectivity and kBET on the latent kNN graph: two scIB integration numbers that are functions of the exact cosine
neighbours `umap.knn_graph` computes (libmmvae_graph.so, include/mmvae_graph.h).

    connected_components   smallest-index root of every vertex of any [N, k] neighbour table (HIP rounds, driven here)
    graph_connectivity     per label class, the share of its cells in the largest component of the graph restricted to it
    kbet                   per cell, the chi-square test of its neighbourhood's batch composition (HIP)
    kbet_per_label         scIB's procedure: one kNN graph and one test per label class
    graph_metrics          the whole call on latent embeddings and their metadata, with a summary table

The definitions are those of include/mmvae_graph.h.  Deviations from scIB's kBET are listed in DESIGN.md: at most 63
neighbours where scIB allows 70, and the cosine distances of the exact graph.

Device tensors run the HIP kernels, always.  CPU tensors are refused outside `backend.cpu_plumbing()`; inside it every
function is its statement in torch ops, fp64 where it computes (tests/graph_restatement.py restates it independently).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import backend
from ._bind import ptr as _ptr, stream as _stream

MAX_K = 64
MAX_BATCHES = 64
MAX_ROUNDS = 64
KBET_MAX_NEIGHBOURS = 63     # scIB caps k0 at 70; the kNN entry holds 64 ranks, the cell included
GAMMA_MAX_TERMS = 500
GAMMA_EPS = 2.0 ** -52
GAMMA_TINY = 1e-300


# ------------------------------------------------------------------------------------------------------- arguments
def _table(idx: torch.Tensor, what: str, min_k: int = 1) -> Tuple[int, int, bool]:
    if idx.dim() != 2:
        raise ValueError(f"{what}: idx must be [N, k], got {tuple(idx.shape)}")
    N, k = idx.shape
    if not (N >= 1 and min_k <= k <= MAX_K):
        raise ValueError(f"{what}: need N >= 1 and {min_k} <= k <= {MAX_K} (got N = {N}, k = {k})")
    if idx.dtype != torch.int32:
        raise ValueError(f"{what}: idx must be int32, got {idx.dtype}")
    return N, k, backend.on_hip(idx)


def _check_indices(idx: torch.Tensor, N: int, what: str) -> None:
    """A caller-made table: the kernels trust idx to lie in [0, N) (one reduction and a host read)."""
    lo, hi = torch.aminmax(idx)
    if int(lo) < 0 or int(hi) >= N:
        raise ValueError(f"{what}: neighbour indices must lie in [0, {N}) (found {int(lo)} .. {int(hi)})")


def _codes(t: Optional[torch.Tensor], N: int, like: torch.Tensor, what: str, name: str = "codes") -> None:
    if t is None:
        return
    if t.dtype != torch.int32:
        raise ValueError(f"{what}: {name} must be int32 (negative = unlabelled), got {t.dtype}")
    if t.shape != (N,):
        raise ValueError(f"{what}: {name} must be [N] with N = {N}, got {tuple(t.shape)}")
    if t.device != like.device:
        raise ValueError(f"{what}: {name} are on {t.device}, the table on {like.device}")


# ----------------------------------------------------------------------------------------------- connected components
def _kept_edges(idx: torch.Tensor, codes: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    N, k = idx.shape
    src = torch.arange(N, device=idx.device).repeat_interleave(k)
    dst = idx.reshape(-1).long()
    keep = src != dst
    if codes is not None:
        keep &= (codes[src] >= 0) & (codes[src] == codes[dst])
    return src[keep], dst[keep]


def _components_torch(idx: torch.Tensor, codes: Optional[torch.Tensor], max_rounds: int) -> Tuple[torch.Tensor, int]:
    """The round in torch ops on idx's device: hook the larger of every kept edge's two parents onto the smaller with
    scatter_reduce(amin), then one hop parent[parent]; the round that changes nothing ends it."""
    src, dst = _kept_edges(idx, codes)
    parent = torch.arange(idx.shape[0], device=idx.device)
    for rounds in range(1, max_rounds + 1):
        a, b = parent[src], parent[dst]
        new = parent.scatter_reduce(0, torch.maximum(a, b), torch.minimum(a, b), "amin")
        new = new[new]
        if torch.equal(new, parent):
            return parent.to(torch.int32), rounds
        parent = new
    raise RuntimeError(f"connected_components: no fixpoint within max_rounds = {max_rounds}")


def connected_components(idx: torch.Tensor, codes: Optional[torch.Tensor] = None, max_rounds: int = MAX_ROUNDS, *,
                         _trusted: bool = False) -> Tuple[torch.Tensor, int]:
    """(root [N] int32, rounds) of the neighbour table idx [N, k] int32: root[i] is the smallest index of i's component
    in the undirected union of the listed edges (self entries and duplicates are ignored).  With `codes` [N] int32 an
    edge counts only between two vertices of one non-negative code; an unlabelled vertex is its own component.

    On the device every round is one `mmvae_graph_cc_round_i32` call, and its `changed` word is read back after EACH
    round (one synchronisation per round).  The first round that wrote nothing ends the call; `rounds` counts it.  The
    result is that fixpoint, which is unique: equal bits on every call, whatever `rounds` was.  RuntimeError once
    `max_rounds` rounds have all written something -- the call never loops unbounded."""
    N, k, hip = _table(idx, "connected_components")
    _codes(codes, N, idx, "connected_components")
    max_rounds = int(max_rounds)
    if max_rounds < 1:
        raise ValueError(f"connected_components: max_rounds must be at least 1 (got {max_rounds})")
    if not _trusted:
        _check_indices(idx, N, "connected_components")
    if not hip:
        return _components_torch(idx, codes, max_rounds)
    from . import _graph_lib

    lib = _graph_lib.load_graph()
    idx = idx.contiguous()
    codes = None if codes is None else codes.contiguous()
    parent = torch.arange(N, dtype=torch.int32, device=idx.device)
    changed = torch.zeros(1, dtype=torch.int32, device=idx.device)
    for rounds in range(1, max_rounds + 1):
        changed.zero_()
        _graph_lib.check(lib.mmvae_graph_cc_round_i32(N, k, _ptr(idx), _ptr(codes), _ptr(parent), _ptr(changed),
                                                      _stream()), "mmvae_graph_cc_round_i32")
        if int(changed) == 0:
            return parent, rounds
    raise RuntimeError(f"connected_components: no fixpoint within max_rounds = {max_rounds}")


def component_sizes(root: torch.Tensor, codes: Optional[torch.Tensor], n_classes: int
                    ) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(class_count [n_classes] int64, class_largest [n_classes] int32, n_components) of the roots `connected_components`
    returns: the labelled vertices per class, the size of each class's largest component and the number of components
    that hold a labelled vertex.  codes = None: one class 0."""
    if root.dim() != 1 or root.dtype != torch.int32 or root.numel() < 1:
        raise ValueError(f"component_sizes: root must be int32 [N], got {root.dtype} {tuple(root.shape)}")
    N = root.numel()
    n_classes = int(n_classes)
    if n_classes < 1 or (codes is None and n_classes != 1):
        raise ValueError(f"component_sizes: n_classes must be at least 1, and 1 without codes (got {n_classes})")
    _codes(codes, N, root, "component_sizes")
    if not backend.on_hip(root):
        c = torch.zeros(N, dtype=torch.int64) if codes is None else codes.long()
        labelled = (c >= 0) & (c < n_classes)
        count = torch.bincount(c[labelled], minlength=n_classes)
        size = torch.bincount(root.long()[labelled], minlength=N)
        is_root = labelled & (root.long() == torch.arange(N))
        largest = torch.zeros(n_classes, dtype=torch.int64).scatter_reduce(0, c[is_root], size[is_root], "amax")
        return count, largest.to(torch.int32), int(is_root.sum())
    from . import _graph_lib

    root = root.contiguous()
    codes = None if codes is None else codes.contiguous()
    size_ws = torch.empty(N, dtype=torch.int32, device=root.device)
    count = torch.empty(n_classes, dtype=torch.int64, device=root.device)
    largest = torch.empty(n_classes, dtype=torch.int32, device=root.device)
    n_comp = torch.empty(1, dtype=torch.int32, device=root.device)
    _graph_lib.check(_graph_lib.load_graph().mmvae_graph_component_sizes_i32(
        N, _ptr(root), _ptr(codes), n_classes, _ptr(size_ws), _ptr(count), _ptr(largest), _ptr(n_comp), _stream()),
        "mmvae_graph_component_sizes_i32")
    return count, largest, int(n_comp)


class Connectivity(NamedTuple):
    per_class: torch.Tensor       # [n_classes] fp64: largest / count, NaN for an empty class
    score: float                  # their mean over the non-empty classes
    n_components: int
    rounds: int
    root: torch.Tensor            # [N] int32
    class_count: torch.Tensor     # [n_classes] int64
    class_largest: torch.Tensor   # [n_classes] int32


def graph_connectivity(idx: torch.Tensor, codes: torch.Tensor, n_classes: int, max_rounds: int = MAX_ROUNDS, *,
                       _trusted: bool = False) -> Connectivity:
    """scIB's graph connectivity of the label `codes` on the table idx: for every class the share of its cells in the
    largest connected component of the graph restricted to that class (NaN for an empty class), their mean over the
    non-empty classes, the number of components over all classes and the rounds `connected_components` took."""
    root, rounds = connected_components(idx, codes, max_rounds, _trusted=_trusted)
    count, largest, n_comp = component_sizes(root, codes, n_classes)
    per = torch.where(count > 0, largest.double() / count.double(), torch.full_like(count, float("nan"), dtype=torch.float64))
    filled = per[count > 0]
    score = float(filled.mean()) if filled.numel() else float("nan")
    return Connectivity(per, score, n_comp, rounds, root, count, largest)


# --------------------------------------------------------------------------------------------------------------- kBET
def _gamma_q_torch(a: float, x: torch.Tensor) -> torch.Tensor:
    """Q(a, x) for x > 0 elementwise in fp64: the series of P below a + 1, the modified Lentz fraction above, each
    element frozen where it meets relative 2^-52 (include/mmvae_graph.h)."""
    front = torch.exp(-x + a * torch.log(x) - math.lgamma(a))
    low = x < a + 1.0
    # the series
    ap = torch.full_like(x, a)
    d = torch.full_like(x, 1.0 / a)
    s = d.clone()
    live = low.clone()
    for _ in range(GAMMA_MAX_TERMS):
        if not bool(live.any()):
            break
        ap = ap + 1.0
        d = torch.where(live, d * (x / ap), d)
        s = torch.where(live, s + d, s)
        live = live & ~(d.abs() < s.abs() * GAMMA_EPS)
    series = 1.0 - s * front
    # the continued fraction
    b = x + 1.0 - a
    c = torch.full_like(x, 1.0 / GAMMA_TINY)
    d = 1.0 / b
    h = d.clone()
    live = ~low
    tiny = torch.full_like(x, GAMMA_TINY)
    for n in range(1, GAMMA_MAX_TERMS + 1):
        if not bool(live.any()):
            break
        an = -n * (n - a)
        b = b + 2.0
        d = an * d + b
        d = torch.where(d.abs() < GAMMA_TINY, tiny, d)
        c = b + an / c
        c = torch.where(c.abs() < GAMMA_TINY, tiny, c)
        d = 1.0 / d
        step = d * c
        h = torch.where(live, h * step, h)
        live = live & ~((step - 1.0).abs() < GAMMA_EPS)
    return torch.where(low, series, front * h)


def _kbet_torch(idx: torch.Tensor, batch: torch.Tensor, freq: torch.Tensor, dof: int) -> Tuple[torch.Tensor, torch.Tensor]:
    B = freq.numel()
    bj = batch[idx[:, 1:].long()]
    counted = (bj >= 0) & (bj < B)
    k_i = counted.sum(1).double()
    stat = torch.zeros_like(k_i)
    for b in range(B):  # ascending, one rounding per operation
        f = float(freq[b])
        if f > 0.0:
            e = k_i * f
            diff = (counted & (bj == b)).sum(1).double() - e
            stat = stat + (diff * diff) / e
    empty = k_i == 0
    nan = torch.full_like(stat, float("nan"))
    stat = torch.where(empty, nan, stat)
    safe = torch.where(empty | (stat == 0), torch.ones_like(stat), stat)
    p = _gamma_q_torch(0.5 * dof, 0.5 * safe)
    return stat, torch.where(empty, nan, torch.where(stat == 0, torch.ones_like(p), p))


def batch_frequencies(batch: torch.Tensor, n_batches: int) -> torch.Tensor:
    """[n_batches] fp64 on the host: the share of every batch among the labelled cells (codes in [0, n_batches))."""
    ok = (batch >= 0) & (batch < n_batches)
    count = torch.bincount(batch[ok].long(), minlength=n_batches).double().cpu()
    return count / count.sum()


def rejection_rate(pval: torch.Tensor, alpha: float = 0.05) -> float:
    """The share of p < alpha among the rows with a defined p (NaN when there is none)."""
    ok = ~torch.isnan(pval)
    n = int(ok.sum())
    return float(((pval < alpha) & ok).sum()) / n if n else float("nan")


def kbet(idx: torch.Tensor, batch: torch.Tensor, freq: Optional[torch.Tensor] = None, alpha: float = 0.05, *,
         _trusted: bool = False) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """(stat [N] fp64, pval [N] fp64, rejection rate) of kBET on the graph idx [N, k] (rank 0 the cell itself, the
    neighbourhood ranks 1 .. k - 1): Pearson's chi-square statistic of every neighbourhood's batch counts against the
    expected shares `freq` [n_batches] (default: the labelled cells' global batch frequencies), its p-value at
    (batches with freq > 0) - 1 degrees of freedom, and the share of p < alpha over the rows with a defined p.  A row
    whose neighbours carry no batch has stat = pval = NaN."""
    N, k, hip = _table(idx, "kbet", min_k=2)
    _codes(batch, N, idx, "kbet", "batch")
    if freq is None:
        n_batches = max(2, int(batch.max()) + 1)
        if n_batches > MAX_BATCHES:
            raise ValueError(f"kbet: at most {MAX_BATCHES} batches (got codes up to {n_batches - 1})")
        freq = batch_frequencies(batch, n_batches)
    else:
        freq = torch.as_tensor(freq, dtype=torch.float64).cpu()
        if freq.dim() != 1 or not (2 <= freq.numel() <= MAX_BATCHES):
            raise ValueError(f"kbet: freq must be [n_batches] with 2 <= n_batches <= {MAX_BATCHES}, got {tuple(freq.shape)}")
    if not bool(torch.isfinite(freq).all()) or bool((freq < 0).any()):
        raise ValueError("kbet: freq must be finite and non-negative (are there cells with a batch?)")
    dof = int((freq > 0).sum()) - 1
    if dof < 1:
        raise ValueError("kbet: need at least two batches with a positive expected share")
    if not _trusted:
        _check_indices(idx, N, "kbet")
    if not hip:
        stat, pval = _kbet_torch(idx, batch, freq, dof)
    else:
        from . import _graph_lib

        idx, batch = idx.contiguous(), batch.contiguous()
        freq_d = freq.to(idx.device)
        stat = torch.empty(N, dtype=torch.float64, device=idx.device)
        pval = torch.empty_like(stat)
        _graph_lib.check(_graph_lib.load_graph().mmvae_graph_kbet_f64(N, k, _ptr(idx), _ptr(batch), freq.numel(),
                                                                      _ptr(freq_d), dof, _ptr(stat), _ptr(pval), _stream()),
                         "mmvae_graph_kbet_f64")
    return stat, pval, rejection_rate(pval, alpha)


class KbetPerLabel(NamedTuple):
    score: float                  # 1 - the mean rejection rate over the tested classes (NaN: none was tested)
    rejection: torch.Tensor       # [n_labels] fp64 on the host, NaN for a skipped class
    k0: torch.Tensor              # [n_labels] int64 on the host, 0 for a skipped class
    tested: torch.Tensor          # [n_labels] bool on the host


def kbet_k0(batch_counts: torch.Tensor, n_cells: int) -> int:
    """scIB's neighbourhood size of one label class from its cells per batch: a quarter of the mean size of the batches
    present, at least 10, at most 63 (scIB: 70) and at most n_cells - 2."""
    present = batch_counts[batch_counts > 0].double()
    return int(min(KBET_MAX_NEIGHBOURS, max(10, int(math.floor(float(present.mean()) / 4.0))), n_cells - 2))


def kbet_per_label(z: torch.Tensor, batch: torch.Tensor, label: torch.Tensor, alpha: float = 0.05, min_cells: int = 10,
                   n_labels: Optional[int] = None, n_batches: Optional[int] = None) -> KbetPerLabel:
    """kBET the way scIB runs it: separately inside every label class.  A class with at least `min_cells` cells and at
    least two batches present gets its own exact cosine kNN graph (`umap.knn_graph` of the class's rows of z, k0 + 1
    neighbours with k0 of `kbet_k0`) and one `kbet` call against the class's own batch frequencies; any other class is
    skipped and reported as NaN.  score = 1 - the mean rejection rate of the tested classes."""
    from .umap import knn_graph

    N = z.shape[0]
    _codes(batch, N, z, "kbet_per_label", "batch")
    _codes(label, N, z, "kbet_per_label", "label")
    min_cells = int(min_cells)
    if min_cells < 3:
        raise ValueError(f"kbet_per_label: min_cells must be at least 3 (got {min_cells})")
    L = int(n_labels) if n_labels is not None else max(1, int(label.max()) + 1)
    B = int(n_batches) if n_batches is not None else max(2, int(batch.max()) + 1)
    if B > MAX_BATCHES:
        raise ValueError(f"kbet_per_label: at most {MAX_BATCHES} batches (got {B})")
    in_class = (label >= 0) & (label < L)
    in_batch = in_class & (batch >= 0) & (batch < B)
    cells = torch.bincount(label[in_class].long(), minlength=L).cpu()
    table = torch.bincount(label[in_batch].long() * B + batch[in_batch].long(), minlength=L * B).view(L, B).cpu()
    rejection = torch.full((L,), float("nan"), dtype=torch.float64)
    k0s = torch.zeros(L, dtype=torch.int64)
    tested = torch.zeros(L, dtype=torch.bool)
    for c in range(L):
        n_c = int(cells[c])
        if n_c < min_cells or int((table[c] > 0).sum()) < 2:
            continue
        k0 = kbet_k0(table[c], n_c)
        rows = torch.nonzero(label == c).squeeze(1)
        idx, _ = knn_graph(z[rows], k0 + 1)
        freq = table[c].double() / table[c].double().sum()
        _, _, rejection[c] = kbet(idx, batch[rows], freq, alpha, _trusted=True)
        k0s[c], tested[c] = k0, True
    score = 1.0 - float(rejection[tested].mean()) if bool(tested.any()) else float("nan")
    return KbetPerLabel(score, rejection, k0s, tested)


# ------------------------------------------------------------------------------------------------------ the whole call
@dataclass
class GraphMetrics:
    """What `graph_metrics` returns.  The per-cell tensors stay on the embeddings' device; the tables are pandas frames
    on the host."""
    idx: torch.Tensor                 # [N, k] int32: the kNN graph the components and the whole-graph kBET were read from
    columns: Tuple[str, ...]          # the batch column first, then the label columns
    codes: torch.Tensor               # [n_columns, N] int32, -1 = missing
    categories: Dict[str, object]     # column -> the pandas Index its codes point into
    kbet_stat: Optional[torch.Tensor]  # [N] fp64 of the whole graph (None: fewer than two batches)
    kbet_pval: Optional[torch.Tensor]
    summary: object                   # DataFrame, one row per label column (SUMMARY_COLUMNS)
    root: Dict[str, torch.Tensor] = field(default_factory=dict)       # label column -> [N] int32
    per_class: Dict[str, object] = field(default_factory=dict)        # label column -> DataFrame (CLASS_COLUMNS)


SUMMARY_COLUMNS = ("column", "n_classes", "n_cells", "graph_connectivity", "n_components", "cc_rounds",
                   "kbet_rejection_global", "kbet_score", "n_classes_tested")
CLASS_COLUMNS = ("class", "n_cells", "largest_component", "connectivity", "kbet_k0", "kbet_rejection", "kbet_tested")


def class_table(names: Sequence, class_count, class_largest, k0, rejection, tested):
    """The per-class table of one label column (CLASS_COLUMNS) from host sequences of one entry per class."""
    import pandas as pd

    rows = []
    for name, n, big, k, rej, ok in zip(names, class_count, class_largest, k0, rejection, tested):
        n, big = int(n), int(big)
        rows.append((name, n, big, big / n if n else float("nan"), int(k), float(rej), bool(ok)))
    return pd.DataFrame(rows, columns=list(CLASS_COLUMNS))


def summary_row(column: str, table, n_components: int, rounds: int, global_rejection: float) -> tuple:
    """One row of the summary (SUMMARY_COLUMNS) from a column's class table: the connectivity is the mean over the
    non-empty classes, the kBET score 1 - the mean rejection over the tested ones (NaN where there is none)."""
    filled = table["connectivity"][table["n_cells"] > 0]
    tested = table["kbet_rejection"][table["kbet_tested"]]
    nan = float("nan")
    return (column, len(table), int(table["n_cells"].sum()), float(filled.mean()) if len(filled) else nan,
            int(n_components), int(rounds), float(global_rejection), 1.0 - float(tested.mean()) if len(tested) else nan,
            len(tested))


def graph_metrics(z: torch.Tensor, metadata, batch_key: str = "species", label_keys: Sequence[str] = ("cell_type",),
                  n_neighbors: int = 15, alpha: float = 0.05) -> GraphMetrics:
    """Graph connectivity and kBET of latent embeddings z [N, D] with one metadata row per cell.

    One `umap.knn_graph(z, n_neighbors)`; on it the connected components of every label column (`graph_connectivity`)
    and one whole-graph `kbet` of the batch column; then `kbet_per_label` per label column, which builds its own graphs.
    Codes come from `mixing.factorize`, NaN = -1.  With fewer than two batches the kBET columns are NaN.  The summary has
    one row per label column (SUMMARY_COLUMNS); per_class[label column] one row per class (CLASS_COLUMNS)."""
    import pandas as pd

    from .mixing import factorize
    from .umap import knn_graph

    if isinstance(label_keys, str):
        label_keys = (label_keys,)
    columns = (batch_key,) + tuple(label_keys)
    missing = [c for c in columns if c not in metadata.columns]
    if missing:
        raise KeyError(f"graph_metrics: metadata has no column {missing} (it has {list(metadata.columns)})")
    if len(metadata) != z.shape[0]:
        raise ValueError(f"graph_metrics: {z.shape[0]} embeddings but {len(metadata)} metadata rows")
    idx, _ = knn_graph(z, n_neighbors)
    factored = [factorize(metadata[c]) for c in columns]
    categories = {c: u for c, (_, u) in zip(columns, factored)}
    codes = torch.stack([f[0] for f in factored]).to(z.device)
    B = len(categories[batch_key])
    if B > MAX_BATCHES:
        raise ValueError(f"graph_metrics: column {batch_key!r} has {B} batches, at most {MAX_BATCHES} are tested")
    stat = pval = None
    global_rejection = float("nan")
    if B >= 2:
        stat, pval, global_rejection = kbet(idx, codes[0], batch_frequencies(codes[0], B), alpha, _trusted=True)
    out = GraphMetrics(idx, columns, codes, categories, stat, pval, None)
    rows = []
    for n, key in enumerate(label_keys, start=1):
        L = len(categories[key])
        if L == 0:
            table = class_table([], [], [], [], [], [])
            rows.append(summary_row(key, table, 0, 0, global_rejection))
            out.per_class[key] = table
            continue
        conn = graph_connectivity(idx, codes[n], L, _trusted=True)
        out.root[key] = conn.root
        if B >= 2:
            per = kbet_per_label(z, codes[0], codes[n], alpha, n_labels=L, n_batches=B)
        else:
            per = KbetPerLabel(float("nan"), torch.full((L,), float("nan"), dtype=torch.float64),
                               torch.zeros(L, dtype=torch.int64), torch.zeros(L, dtype=torch.bool))
        table = class_table(list(categories[key]), conn.class_count.cpu().tolist(), conn.class_largest.cpu().tolist(),
                            per.k0.tolist(), per.rejection.tolist(), per.tested.tolist())
        out.per_class[key] = table
        rows.append(summary_row(key, table, conn.n_components, conn.rounds, global_rejection))
    out.summary = pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS))
    return out


def _display(v):
    return v.decode() if isinstance(v, bytes) else v


def write_tables(result: GraphMetrics, save_dir: str, key: str) -> list:
    """`save_dir`/graph_metrics.{key}.csv (the summary) and one graph_metrics.{key}.{label column}.csv per label column
    (its classes); the paths."""
    import os

    os.makedirs(save_dir, exist_ok=True)
    paths = [os.path.join(save_dir, f"graph_metrics.{key}.csv")]
    result.summary.to_csv(paths[0], index=False)
    for name, table in result.per_class.items():
        paths.append(os.path.join(save_dir, f"graph_metrics.{key}.{name}.csv"))
        table.assign(**{"class": table["class"].map(_display)}).to_csv(paths[-1], index=False)
    return paths


def metrics_from_predictions(directory: str, keys: Sequence[str], batch_key: str = "species",
                             label_keys: Sequence[str] = ("cell_type",), save_dir: Optional[str] = None, **kw) -> list:
    """`graph_metrics` of stored predictions, in the two input forms of `mixing.metrics_from_predictions`: a directory
    holding `{key}_embeddings.npz` with `{key}_metadata.pkl`, or a predictions.h5 read through
    `predictions.load_from_hdf5`.  Writes the tables of `write_tables` into `save_dir` (default: the directory, or the
    file's) and returns their paths."""
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
        result = graph_metrics(_as_points(X), metadata, batch_key, label_keys, **kw)
        paths += write_tables(result, out_dir, key)
    return paths
