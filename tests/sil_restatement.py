"""An independent numpy fp64 restatement of the definitions of include/mmvae_sil.h: a loop over rows with direct
differences sum (x_i - x_j)^2 -- no Gram form, no sorting.  It shares no code with mmvae_amd/silhouette.py.  A helper
module of tests/test_silhouette_host.py and tests/test_silhouette_gpu.py.

It works on unsorted (cls, group) codes, negative = unlabelled, and beside every result it says how far `nearest` can be
trusted: lead[i] is by how much the second-best other class's mean exceeds the best one's (inf with fewer than two).
"""
import numpy as np


# ------------------------------------------------------------------------------------------------------------ inputs
def clusters(seed, n, dim, n_classes, shift=3.0, spread=1.2, centre_scale=3.0):
    """(points, class of every point): Gaussian blobs around random centres, every coordinate shifted by `shift`.  The
    centres are as far from each other as the shift is long, so that the classes also differ in direction (cosine)."""
    rng = np.random.default_rng(seed)
    centres = centre_scale * rng.standard_normal((n_classes, dim))
    which = rng.integers(0, n_classes, n)
    return centres[which] + spread * rng.standard_normal((n, dim)) + shift, which.astype(np.int32)


def with_duplicates(X, cls, of_class=0):
    """Every cell of class `of_class` becomes a copy of the first of them."""
    X = X.copy()
    members = np.nonzero(cls == of_class)[0]
    if len(members):
        X[members] = X[members[0]]
    return X


def sorted_runs(cls, group=None):
    """(order, run_ptr, run_group, run_class) by numpy's lexsort: the kept cells (codes >= 0) sorted stably by
    (group, class) -- the input layout of include/mmvae_sil.h."""
    cls = np.asarray(cls)
    group = np.zeros_like(cls) if group is None else np.asarray(group)
    kept = np.nonzero((cls >= 0) & (group >= 0))[0]
    order = kept[np.lexsort((kept, cls[kept], group[kept]))]
    c, g = cls[order], group[order]
    starts = [0] + [i for i in range(1, len(order)) if c[i] != c[i - 1] or g[i] != g[i - 1]]
    run_ptr = np.array(starts + [len(order)], dtype=np.int32)
    return order, run_ptr, g[starts].astype(np.int32), c[starts].astype(np.int32)


# ------------------------------------------------------------------------------------------------------- definitions
def distances_from(X, i, metric, U=None):
    if metric == "euclidean":
        diff = X - X[i]
        return np.sqrt((diff * diff).sum(1))
    return np.maximum(1.0 - U @ U[i], 0.0)


def silhouette(X, cls, group=None, metric="euclidean"):
    """(a, b, s fp64 [N], nearest int32 [N] class codes, lead fp64 [N]) of rows X (read as fp64) with class codes `cls`
    and group codes `group` (None: one group).  Cells with a negative code get NaN / -1 and belong to no mean."""
    X = np.asarray(X, dtype=np.float64)
    cls = np.asarray(cls)
    group = np.zeros_like(cls) if group is None else np.asarray(group)
    N = len(X)
    U = None
    if metric == "cosine":
        norm = np.sqrt((X * X).sum(1))
        U = X * np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 0.0)[:, None]
    a, b, s = (np.full(N, np.nan) for _ in range(3))
    nearest = np.full(N, -1, dtype=np.int32)
    lead = np.full(N, np.inf)
    kept = (cls >= 0) & (group >= 0)
    for i in range(N):
        if not kept[i]:
            continue
        d = distances_from(X, i, metric, U)
        peers = kept & (group == group[i])
        own = peers & (cls == cls[i])
        own[i] = False
        n_own = int(own.sum()) + 1
        a[i] = d[own].sum() / (n_own - 1) if n_own > 1 else 0.0
        means = sorted((d[peers & (cls == c)].mean(), int(c)) for c in np.unique(cls[peers]) if c != cls[i])
        if not means:
            continue
        b[i], nearest[i] = means[0]
        if len(means) > 1:
            lead[i] = means[1][0] - means[0][0]
        top = max(a[i], b[i])
        s[i] = 0.0 if (n_own == 1 or top == 0.0) else (b[i] - a[i]) / top
    return a, b, s, nearest, lead


def gram_form_fp32(X32, cls, group=None):
    """(a, b) fp64 of the Euclidean FORMULA of the header evaluated in fp32 on the host: g_ij by an fp32 chain over the
    columns, n_i = g_ii, d = sqrt(max(0, n_i + n_j - 2 g_ij)) in fp32 with the distance of bit-equal rows 0 (which the
    header's norm rule guarantees), the means in fp64.  The error of this against `silhouette` is the formula's own."""
    X32 = np.asarray(X32, dtype=np.float32)
    cls = np.asarray(cls)
    group = np.zeros_like(cls) if group is None else np.asarray(group)
    N = len(X32)
    G = np.zeros((N, N), dtype=np.float32)
    same = np.ones((N, N), dtype=bool)
    for k in range(X32.shape[1]):
        G += X32[:, k:k + 1] * X32[None, :, k]
        same &= X32[:, k:k + 1] == X32[None, :, k]
    n = np.diag(G).copy()
    Dm = np.sqrt(np.maximum((n[:, None] + n[None, :]) - np.float32(2.0) * G, np.float32(0.0))).astype(np.float64)
    Dm[same] = 0.0
    a, b = np.full(N, np.nan), np.full(N, np.nan)
    kept = (cls >= 0) & (group >= 0)
    for i in range(N):
        if not kept[i]:
            continue
        peers = kept & (group == group[i])
        own = peers & (cls == cls[i])
        own[i] = False
        a[i] = Dm[i, own].mean() if own.any() else 0.0
        means = [Dm[i, peers & (cls == c)].mean() for c in np.unique(cls[peers]) if c != cls[i]]
        if means:
            b[i] = min(means)
    return a, b


# --------------------------------------------------------------------------------------------------------- averages
def asw_label(s):
    return float(np.nanmean(s))


def asw_batch(s, label, batch):
    """scIB's silhouette_batch: per label the mean of 1 - |s| (labels with one batch, or with as many batches as cells,
    are left out), then the mean over the labels."""
    per = []
    for c in np.unique(label[label >= 0]):
        cells = (label == c) & (batch >= 0)
        n_batches = len(np.unique(batch[cells]))
        if n_batches == 1 or n_batches == cells.sum():
            continue
        per.append(float(np.mean(1.0 - np.abs(s[cells]))))
    return float(np.mean(per)) if per else float("nan")
