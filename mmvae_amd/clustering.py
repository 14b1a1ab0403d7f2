"""K-means clusters of latent embeddings and how well they recover the annotation: the "NMI / ARI cluster / label" pair
of the scIB benchmark (Luecken et al. 2022), next to the kNN-graph metrics of `mmvae_amd.mixing` and the silhouette widths
of `mmvae_amd.silhouette` (libmmvae_clust.so, include/mmvae_clust.h).

    kmeans_step               one Lloyd iteration: labels, squared distances, counts, the new centroids, the record (HIP)
    kmeans_seed               k-means++ rows from given uniforms (the distance pass is HIP)
    kmeans_fit                centring, seeding, the Lloyd loop with relocation of empty clusters, n_init runs
    contingency               the clusters x classes table of two code vectors
    adjusted_rand_index       ARI of such a table
    normalized_mutual_info    NMI of such a table (arithmetic-mean normalisation)
    cluster_metrics           the whole call on latent embeddings and their metadata, with summary tables
    write_tables, clusters_from_predictions

The definitions are those of include/mmvae_clust.h.  Device tensors run the HIP kernels, always.  CPU tensors are refused
outside `backend.cpu_plumbing()`; inside it every function is its statement in fp64 (tests/kmeans_restatement.py restates
it independently).

Where this differs from scikit-learn's KMeans and scib-metrics' nmi_ari_cluster_labels_kmeans: the device scores rows by
the Gram form n + m - 2 g on centred rows (scikit-learn: the same form, without the fp64 centring); the seeding is plain
k-means++ (one draw per round, not the greedy 2 + log C candidates); an empty cluster is moved to the row farthest from its
centroid, chosen by (largest dist2, smallest index), and that row is not taken out of its old cluster's mean.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import backend
from ._bind import ptr as _ptr, stream as _stream

MAX_D = 512
MAX_C = 256
STATS_BYTES = 24


class KMeansStats(NamedTuple):
    """The record of one Lloyd iteration, on the host: the fp64 sum of dist2, sum_c |new_c - old_c|^2, the rows whose
    label changed, the clusters without a row."""
    inertia: float
    shift2: float
    changed: int
    empty: int


@dataclass
class KMeansResult:
    """What `kmeans_fit` returns.  Tensors are on the rows' device."""
    labels: torch.Tensor          # [N] int32
    centroids: torch.Tensor       # [C, D] in the caller's coordinates (fp32 on the device, fp64 on CPU plumbing)
    inertia: float                # sum of squared distances of the rows to their centroids
    n_iter: int                   # Lloyd iterations of the winning run
    converged: bool
    counts: torch.Tensor          # [C] int32 rows per cluster
    history: Tuple[float, ...] = ()   # the inertia every iteration of the winning run reported
    offset: Optional[torch.Tensor] = None     # [1, D] fp64: the column mean the rows were centred on
    centred: Optional[torch.Tensor] = None    # [C, D]: the centroids as the iterations saw them (centroids - offset)


# ------------------------------------------------------------------------------------------------ the fp64 statements
def _step_torch(x: torch.Tensor, centroids: torch.Tensor, label: torch.Tensor):
    x, cen = x.double(), centroids.double()
    d2 = torch.stack([((x - c) ** 2).sum(1) for c in cen], 1)
    dist2, new_label = d2.min(1)  # (the first minimum: ties go to the smaller index)
    C = cen.shape[0]
    counts = torch.bincount(new_label, minlength=C)
    sums = torch.zeros_like(cen).index_add_(0, new_label, x)
    new = torch.where((counts > 0)[:, None], sums / counts.clamp_min(1)[:, None].double(), cen)
    stats = KMeansStats(float(dist2.sum()), float(((new - cen) ** 2).sum()), int((new_label != label.long()).sum()),
                        int((counts == 0).sum()))
    return new, new_label.to(torch.int32), dist2, counts.to(torch.int32), stats


def _seed_update_torch(x: torch.Tensor, row: int, first: bool, mind2: Optional[torch.Tensor]) -> torch.Tensor:
    e = ((x.double() - x[row].double()) ** 2).sum(1)
    return e if first else torch.minimum(mind2, e)


# ------------------------------------------------------------------------------------------------------ 1. the entries
def _check_rows(x: torch.Tensor, what: str) -> None:
    if x.dim() != 2 or not (x.shape[0] >= 1 and 1 <= x.shape[1] <= MAX_D):
        raise ValueError(f"{what}: x must be [N, D] with N >= 1 and 1 <= D <= {MAX_D}, got {tuple(x.shape)}")


def _device_rows(x: torch.Tensor, what: str) -> Tuple[torch.Tensor, int]:
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32 rows, got {x.dtype}")
    n, D = x.shape
    if x.stride(1) != 1 or (n > 1 and x.stride(0) < D):
        x = x.contiguous()
    return x, (x.stride(0) if n > 1 else D)


class _StepBuffers:
    """The outputs and the workspace of mmvae_clust_kmeans_step_f32 at one shape, allocated once for a whole fit."""

    def __init__(self, lib, n: int, D: int, C: int, device):
        self.nbytes = lib.mmvae_clust_kmeans_workspace_bytes(n, D, C)
        if self.nbytes == 0:
            raise ValueError(f"kmeans: libmmvae_clust.so refuses the shape N = {n}, D = {D}, C = {C}")
        self.workspace = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.stats = torch.empty(STATS_BYTES // 8, dtype=torch.float64, device=device)
        self.dist2 = torch.empty(n, dtype=torch.float32, device=device)
        self.counts = torch.empty(C, dtype=torch.int32, device=device)

    def read_stats(self) -> KMeansStats:
        return KMeansStats(*struct.unpack("<ddii", bytes(self.stats.view(torch.uint8).cpu().numpy())))


def _step_device(lib, x, ldx, centroids, new_centroids, label, buf: _StepBuffers) -> None:
    from . import _clust_lib

    n, D = x.shape
    _clust_lib.check(lib.mmvae_clust_kmeans_step_f32(n, D, _ptr(x), ldx, centroids.shape[0], _ptr(centroids),
                                                     _ptr(new_centroids), _ptr(label), _ptr(buf.dist2), _ptr(buf.counts),
                                                     _ptr(buf.stats), _ptr(buf.workspace), buf.nbytes, _stream()),
                     "mmvae_clust_kmeans_step_f32")


def kmeans_step(x: torch.Tensor, centroids: torch.Tensor, label: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, KMeansStats]:
    """(new_centroids [C, D], label [N] int32, dist2 [N], counts [C] int32, stats) of one Lloyd iteration -- the entry of
    include/mmvae_clust.h as it stands: no centring.  x [N, D] float32 with unit column stride (any row stride >= D),
    centroids [C, D]; `label` the labels of the iteration before (None: all -1), left as it is.  The seam under
    `kmeans_fit`, and what tools/bench_kmeans.py times.  On the device dist2 and the centroids are fp32, as the library
    stores them; on CPU plumbing they are the fp64 statement, unrounded."""
    _check_rows(x, "kmeans_step")
    n, D = x.shape
    if centroids.dim() != 2 or centroids.shape[1] != D or not 1 <= centroids.shape[0] <= min(n, MAX_C):
        raise ValueError(f"kmeans_step: centroids must be [C, {D}] with 1 <= C <= min(N, {MAX_C}), got "
                         f"{tuple(centroids.shape)}")
    if centroids.device != x.device or (label is not None and label.device != x.device):
        raise TypeError("kmeans_step: the centroids and the labels must be on the rows' device")
    if label is not None and (label.shape != (n,) or label.dtype != torch.int32):
        raise ValueError("kmeans_step: label must be [N] int32")
    if label is None:
        label = torch.full((n,), -1, dtype=torch.int32, device=x.device)
    if not backend.on_hip(x):
        return _step_torch(x, centroids, label)
    from . import _clust_lib

    lib = _clust_lib.load_clust()
    x, ldx = _device_rows(x, "kmeans_step")
    if centroids.dtype != torch.float32:
        raise TypeError(f"kmeans_step: expected float32 centroids, got {centroids.dtype}")
    centroids = centroids.contiguous()
    buf = _StepBuffers(lib, n, D, centroids.shape[0], x.device)
    new, label = torch.empty_like(centroids), label.clone()
    _step_device(lib, x, ldx, centroids, new, label, buf)
    return new, label, buf.dist2, buf.counts, buf.read_stats()


def _seed_update(x: torch.Tensor, ldx: int, row: int, first: bool, mind2: Optional[torch.Tensor], hip: bool) -> torch.Tensor:
    if not hip:
        return _seed_update_torch(x, row, first, mind2)
    from . import _clust_lib

    lib = _clust_lib.load_clust()
    if mind2 is None:
        mind2 = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _clust_lib.check(lib.mmvae_clust_seed_update_f32(x.shape[0], x.shape[1], _ptr(x), ldx, int(row), int(first),
                                                     _ptr(mind2), _stream()), "mmvae_clust_seed_update_f32")
    return mind2


def seed_distances(x: torch.Tensor, row: int, mind2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mind2 [N]: the squared distance of every row of x to row `row` (mind2 None), or the smaller of that and the given
    mind2, which is updated in place on the device -- one seeding pass of include/mmvae_clust.h."""
    _check_rows(x, "seed_distances")
    if not 0 <= row < x.shape[0]:
        raise ValueError(f"seed_distances: row must be in [0, {x.shape[0]}), got {row}")
    hip = backend.on_hip(x)
    ldx = x.shape[1]
    if hip:
        x, ldx = _device_rows(x, "seed_distances")
    return _seed_update(x, ldx, row, mind2 is None, mind2, hip)


def kmeans_seed(x: torch.Tensor, n_clusters: int, uniforms) -> torch.Tensor:
    """rows [C] int64 (on the host): the k-means++ seeding of Arthur & Vassilvitskii from C given uniforms in [0, 1).  The
    first row is floor(u_0 N).  Round k = 1 .. C - 1 updates every row's squared distance to the nearest chosen row (one
    launch) and draws the first row whose fp64 cumulative sum of those distances exceeds u_k times their total; when the
    total is 0 (every remaining row is a copy of a chosen one) it takes the first row not yet chosen."""
    import numpy as np

    _check_rows(x, "kmeans_seed")
    n = x.shape[0]
    C = int(n_clusters)
    u = np.asarray(uniforms, dtype=np.float64)
    if not 1 <= C <= min(n, MAX_C):
        raise ValueError(f"kmeans_seed: n_clusters must be in [1, min(N, {MAX_C})], got {C}")
    if u.shape != (C,) or not ((u >= 0) & (u < 1)).all():
        raise ValueError(f"kmeans_seed: uniforms must be [{C}] values in [0, 1)")
    hip = backend.on_hip(x)
    ldx = x.shape[1]
    if hip:
        x, ldx = _device_rows(x, "kmeans_seed")
    rows = [min(int(u[0] * n), n - 1)]
    mind2 = None
    for k in range(1, C):
        mind2 = _seed_update(x, ldx, rows[-1], k == 1, mind2, hip)
        cum = torch.cumsum(mind2.double(), 0)
        total = float(cum[-1])
        if total > 0.0:
            at = torch.searchsorted(cum, torch.tensor([u[k] * total], dtype=torch.float64, device=x.device), right=True)
            rows.append(min(int(at[0]), n - 1))
        else:
            taken = set(rows)
            rows.append(next(i for i in range(n) if i not in taken))
    return torch.tensor(rows, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------------ 2. the fit
def _relocate(new: torch.Tensor, counts: torch.Tensor, dist2: torch.Tensor, x: torch.Tensor) -> None:
    """Every cluster without a row, in ascending order, moves onto the row with the largest dist2 not used yet (ties: the
    smaller index)."""
    d = dist2.clone()
    for c in torch.nonzero(counts == 0).flatten().tolist():
        row = int(torch.nonzero(d == d.max())[0])
        new[c] = x[row].to(new.dtype)
        d[row] = -1.0


def _one_run(x, ldx, C, uniforms, max_iter, tol_abs, hip):
    n, D = x.shape
    rows = kmeans_seed(x, C, uniforms)
    cen = x[rows.to(x.device)].contiguous()
    label = torch.full((n,), -1, dtype=torch.int32, device=x.device)
    if hip:
        from . import _clust_lib

        lib = _clust_lib.load_clust()
        buf = _StepBuffers(lib, n, D, C, x.device)
        new = torch.empty_like(cen)

        def step(cen, new, label):
            _step_device(lib, x, ldx, cen, new, label, buf)  # (label is updated in place)
            return new, label, buf.dist2, buf.counts, buf.read_stats()
    else:
        new = None

        def step(cen, new, label):
            return _step_torch(x, cen, label)
    history, converged, n_iter, settled = [], False, 0, False
    for n_iter in range(1, max_iter + 1):
        out, label, dist2, counts, stats = step(cen, new, label)
        history.append(stats.inertia)
        if stats.empty > 0:
            _relocate(out, counts, dist2, x)
        cen, new = out, cen
        if stats.empty == 0 and stats.changed == 0:
            converged = settled = True
            break
        if stats.empty == 0 and stats.shift2 <= tol_abs:
            converged = True
            break
    if not settled:  # the labels belong to the centroids before the last update: one more assignment, its means unused
        _, label, dist2, counts, stats = step(cen, new, label)
    return KMeansResult(label.clone(), cen.clone(), stats.inertia, n_iter, converged, counts.clone(), tuple(history))


def kmeans_fit(x: torch.Tensor, n_clusters: int, seed: int = 0, n_init: int = 1, max_iter: int = 300, tol: float = 1e-4
               ) -> KMeansResult:
    """K-means of the rows x [N, D] with `n_clusters` <= min(N, 256) clusters.

    The rows are centred on their fp64 column mean (and on the device rounded to fp32) before any launch: a translation
    changes no distance and shrinks the cancellation of the Gram form.  Run r of `n_init` seeds with `kmeans_seed` from
    the r-th block of n_clusters uniforms of numpy.random.default_rng(seed), so that a seed means the same fit
    everywhere.  Every Lloyd iteration is one `mmvae_clust_kmeans_step_f32` and one 24-byte read of its record.  After an
    iteration that left clusters empty each of them moves onto the row farthest from its centroid (largest dist2 not used
    yet, ties to the smaller index) and the loop goes on; otherwise it stops when no label changed, or when
    shift2 <= tol x the mean column variance (scikit-learn's rule), or after max_iter iterations.  Unless it stopped on
    unchanged labels, one more assignment makes the labels those of the returned centroids.  The run with the smallest
    inertia wins; an earlier run wins ties.  `centroids` are in the caller's coordinates; `centred` and `offset` are the
    centroids and the column mean as the iterations saw them (`kmeans_step((x - offset).float(), centred, labels)`
    reproduces the last assignment bit for bit)."""
    import numpy as np

    _check_rows(x, "kmeans_fit")
    n, D = x.shape
    C = int(n_clusters)
    if not 1 <= C <= min(n, MAX_C):
        raise ValueError(f"kmeans_fit: n_clusters must be in [1, min(N, {MAX_C})], got {C}")
    if n_init < 1 or max_iter < 1:
        raise ValueError("kmeans_fit: n_init and max_iter must be at least 1")
    hip = backend.on_hip(x)
    if hip and x.dtype != torch.float32:
        raise TypeError(f"kmeans_fit: expected float32 rows, got {x.dtype}")
    x64 = x.double()
    mean = x64.mean(0, keepdim=True)
    rows = x64 - mean
    tol_abs = float(tol) * float(rows.var(0, unbiased=False).mean())
    ldx = D
    if hip:
        rows = rows.float().contiguous()
    del x64
    rng = np.random.default_rng(seed)
    best = None
    for _ in range(n_init):
        run = _one_run(rows, ldx, C, rng.random(C), max_iter, tol_abs, hip)
        if best is None or run.inertia < best.inertia:
            best = run
    best.offset, best.centred = mean, best.centroids
    best.centroids = (best.centred.double() + mean).to(rows.dtype)
    return best


# ------------------------------------------------------------------------------------------------------ 3. agreement
def contingency(a: torch.Tensor, b: torch.Tensor, n_a: Optional[int] = None, n_b: Optional[int] = None) -> torch.Tensor:
    """table [n_a, n_b] int64 on the codes' device: the rows with a[i] = r and b[i] = c, through torch.bincount.  Rows
    with a negative code on either side are left out.  n_a, n_b default to the largest code + 1."""
    if a.dim() != 1 or a.shape != b.shape:
        raise ValueError("contingency: a and b must be [N]")
    for t in (a, b):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"contingency: codes must be int32 or int64 (negative = unlabelled), got {t.dtype}")
    if a.device != b.device:
        raise TypeError(f"contingency: a is on {a.device}, b on {b.device}")
    keep = (a >= 0) & (b >= 0)
    a, b = a[keep].long(), b[keep].long()
    n_a = int(n_a) if n_a is not None else (int(a.max()) + 1 if a.numel() else 0)
    n_b = int(n_b) if n_b is not None else (int(b.max()) + 1 if b.numel() else 0)
    if a.numel() and (int(a.max()) >= n_a or int(b.max()) >= n_b):
        raise ValueError("contingency: a code exceeds the given number of classes")
    return torch.bincount(a * n_b + b, minlength=n_a * n_b).reshape(n_a, n_b)


def _table(table):
    import numpy as np

    t = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    if t.ndim != 2:
        raise ValueError("a contingency table must be [clusters, classes]")
    return t.astype(np.int64)


def adjusted_rand_index(table) -> float:
    """ARI (Hubert & Arabie) of a contingency table, from the pair counts in exact integers and one fp64 division; 1.0
    where both partitions put every pair the same way (scikit-learn's convention), NaN for an empty table."""
    t = _table(table)
    n = int(t.sum())
    if n == 0:
        return float("nan")
    squares = sum(int(v) ** 2 for v in t.ravel())
    rows = sum(int(v) ** 2 for v in t.sum(1))
    cols = sum(int(v) ** 2 for v in t.sum(0))
    tp, fp, fn = squares - n, cols - squares, rows - squares
    tn = n * n - fp - fn - squares
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def normalized_mutual_info(table) -> float:
    """NMI of a contingency table in fp64: the mutual information over the arithmetic mean of the two entropies
    (scikit-learn's default, scIB's choice).  1.0 where both sides are a single class, 0.0 where the mutual information
    is 0, NaN for an empty table."""
    import numpy as np

    t = _table(table).astype(np.float64)
    n = t.sum()
    if n == 0:
        return float("nan")
    a, b = t.sum(1), t.sum(0)
    if (a > 0).sum() == 1 and (b > 0).sum() == 1:
        return 1.0
    i, j = np.nonzero(t)
    nij = t[i, j]
    mi = float(np.sum(nij / n * (np.log(nij) - np.log(a[i]) - np.log(b[j]) + np.log(n))))
    if mi <= 0.0:
        return 0.0
    ha = -float(np.sum(a[a > 0] / n * (np.log(a[a > 0]) - np.log(n))))
    hb = -float(np.sum(b[b > 0] / n * (np.log(b[b > 0]) - np.log(n))))
    return mi / (0.5 * (ha + hb))


# ------------------------------------------------------------------------------------------------------ 4. whole call
@dataclass
class ClusterMetrics:
    """What `cluster_metrics` returns.  The fits stay on the embeddings' device; the tables are pandas frames on the host."""
    columns: Tuple[str, ...]
    codes: torch.Tensor                       # [n_columns, N] int32, -1 = missing
    categories: Dict[str, object]             # column -> the pandas Index its codes point into
    summary: object                           # DataFrame, one row per label column
    fits: Dict[str, KMeansResult] = field(default_factory=dict)        # label column -> its k-means
    contingency: Dict[str, object] = field(default_factory=dict)       # label column -> DataFrame clusters x categories


SUMMARY_COLUMNS = ("column", "n_clusters", "n_cells", "nmi", "ari", "inertia", "n_iter", "converged")


def cluster_metrics(z: torch.Tensor, metadata, label_keys: Sequence[str] = ("cell_type",), n_clusters: Optional[int] = None,
                    seed: int = 0, n_init: int = 1, max_iter: int = 300) -> ClusterMetrics:
    """NMI and ARI between k-means clusters of the latent embeddings z [N, D] and every label column of the metadata.

    Codes come from `mixing.factorize` (NaN = -1).  Per label column one `kmeans_fit` of ALL cells with `n_clusters`
    clusters (default: the column's number of categories); the library's limit of 256 clusters (and N) caps that number,
    and the summary's n_clusters is the number used.  The contingency table and the two scores leave out the cells
    without a label; n_cells counts the others.  The summary has SUMMARY_COLUMNS, one row per label column."""
    import pandas as pd

    from .mixing import factorize

    if isinstance(label_keys, str):
        label_keys = (label_keys,)
    columns = tuple(label_keys)
    missing = [c for c in columns if c not in metadata.columns]
    if missing:
        raise KeyError(f"cluster_metrics: metadata has no column {missing} (it has {list(metadata.columns)})")
    if len(metadata) != z.shape[0]:
        raise ValueError(f"cluster_metrics: {z.shape[0]} embeddings but {len(metadata)} metadata rows")
    backend.on_hip(z)
    factored = [factorize(metadata[c]) for c in columns]
    categories = {c: u for c, (_, u) in zip(columns, factored)}
    codes = torch.stack([f[0] for f in factored]).to(z.device)
    out = ClusterMetrics(columns, codes, categories, None)
    rows = []
    for n, key in enumerate(columns):
        L = len(categories[key])
        C = max(1, min(int(n_clusters) if n_clusters is not None else L, MAX_C, z.shape[0]))
        fit = kmeans_fit(z, C, seed=seed, n_init=n_init, max_iter=max_iter)
        table = contingency(fit.labels, codes[n], C, L)
        out.fits[key] = fit
        out.contingency[key] = pd.DataFrame(table.cpu().numpy(), index=pd.RangeIndex(C, name="cluster"),
                                            columns=pd.Index(list(categories[key]), name=key))
        rows.append((key, C, int(table.sum()), normalized_mutual_info(table), adjusted_rand_index(table), fit.inertia,
                     fit.n_iter, fit.converged))
    out.summary = pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS))
    return out


def _display(v):
    return v.decode() if isinstance(v, bytes) else v


def write_tables(result: ClusterMetrics, save_dir: str, key: str) -> list:
    """`save_dir`/clusters.{key}.csv (the summary) and per label column clusters.{key}.{column}.contingency.csv and
    clusters.{key}.{column}.labels.npy (the cluster of every cell, int32); the paths."""
    import os

    import numpy as np

    os.makedirs(save_dir, exist_ok=True)
    paths = [os.path.join(save_dir, f"clusters.{key}.csv")]
    result.summary.to_csv(paths[0], index=False)
    for name in result.columns:
        paths.append(os.path.join(save_dir, f"clusters.{key}.{name}.contingency.csv"))
        result.contingency[name].rename(columns=_display).to_csv(paths[-1])
        paths.append(os.path.join(save_dir, f"clusters.{key}.{name}.labels.npy"))
        np.save(paths[-1], result.fits[name].labels.cpu().numpy())
    return paths


def clusters_from_predictions(directory: str, keys: Sequence[str], label_keys: Sequence[str] = ("cell_type",),
                              save_dir: Optional[str] = None, **kw) -> list:
    """`cluster_metrics` of stored predictions, in the two input forms of `silhouette.widths_from_predictions`: a
    directory holding `{key}_embeddings.npz` with `{key}_metadata.pkl`, or a predictions.h5.  Writes the files of
    `write_tables` into `save_dir` (default: the directory, or the file's) and returns their paths."""
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
        result = cluster_metrics(_as_points(X), metadata, label_keys, **kw)
        paths += write_tables(result, out_dir, key)
    return paths
