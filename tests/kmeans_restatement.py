"""An independent numpy fp64 restatement of the definitions of include/mmvae_clust.h and of the fit loop of
mmvae_amd/clustering.py: assignment by the direct form sum (x - c)^2 -- no Gram form --, the update, k-means++ from given
uniforms, the Lloyd loop with the relocation of empty clusters, and ARI and NMI from their textbook formulas.  It shares
no code with mmvae_amd/clustering.py.  A helper module of tests/test_clustering_host.py and tests/test_clustering_gpu.py.

Beside every assignment it says how far a label can be trusted: lead[i] is by how much the second-best centroid's squared
distance exceeds the best one's (inf with a single centroid).
"""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------------- one iteration
def assign(X, centroids):
    """(label int32 [N], d2 fp64 [N], lead fp64 [N]): the nearest centroid of every row (ties: the smaller index)."""
    X, cen = np.asarray(X, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    N, C = len(X), len(cen)
    best = np.full(N, np.inf)
    second = np.full(N, np.inf)
    label = np.zeros(N, dtype=np.int32)
    for c in range(C):
        diff = X - cen[c]
        d = (diff * diff).sum(1)
        better = d < best
        second = np.where(better, best, np.minimum(second, d))
        label[better] = c
        best = np.where(better, d, best)
    return label, best, second - best


def update(X, label, centroids):
    """(new centroids fp64 [C, D], counts [C]): the mean of every cluster's rows; a cluster without a row keeps its
    centroid."""
    X, cen = np.asarray(X, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    new, counts = cen.copy(), np.zeros(len(cen), dtype=np.int64)
    for c in range(len(cen)):
        members = label == c
        counts[c] = members.sum()
        if counts[c]:
            new[c] = X[members].sum(0) / counts[c]
    return new, counts


def step(X, centroids, old_label=None):
    """One Lloyd iteration: a dict of label, d2, lead, counts, new, inertia, shift2, changed, empty."""
    label, d2, lead = assign(X, centroids)
    new, counts = update(X, label, centroids)
    old = np.full(len(label), -1) if old_label is None else np.asarray(old_label)
    shift = new - np.asarray(centroids, dtype=np.float64)
    return dict(label=label, d2=d2, lead=lead, counts=counts, new=new, inertia=float(d2.sum()),
                shift2=float((shift * shift).sum()), changed=int((label != old).sum()), empty=int((counts == 0).sum()))


# ------------------------------------------------------------------------------------------------------------ seeding
def seed(X, n_clusters, uniforms):
    """(rows [C] int64, margin): k-means++ from the given uniforms.  The first row is floor(u_0 N); round k draws the
    first row whose cumulative sum of squared distances to the nearest chosen row exceeds u_k times the total (total 0:
    the first row not chosen yet).  margin is the smallest distance of a threshold from an edge of the cumulative sum,
    as a share of the total (inf with one cluster)."""
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    rows = [min(int(uniforms[0] * N), N - 1)]
    mind2 = np.full(N, np.inf)
    margin = np.inf
    for k in range(1, n_clusters):
        diff = X - X[rows[-1]]
        mind2 = np.minimum(mind2, (diff * diff).sum(1))
        cum = np.cumsum(mind2)
        total = cum[-1]
        if total > 0:
            threshold = uniforms[k] * total
            at = 0
            while at < N - 1 and not cum[at] > threshold:
                at += 1
            rows.append(at)
            margin = min(margin, np.abs(cum - threshold).min() / total)
        else:
            rows.append(next(i for i in range(N) if i not in rows))
    return np.array(rows, dtype=np.int64), margin


# ---------------------------------------------------------------------------------------------------------------- fit
def centred(X, round32):
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(0, keepdims=True)
    return Xc.astype(np.float32).astype(np.float64) if round32 else Xc


def relocate(X, new, counts, d2):
    d = d2.copy()
    for c in np.nonzero(counts == 0)[0]:
        row = int(np.nonzero(d == d.max())[0][0])
        new[c] = X[row]
        d[row] = -1.0


def fit_run(Xc, n_clusters, uniforms, max_iter, tol_abs):
    rows, _ = seed(Xc, n_clusters, uniforms)
    cen = Xc[rows].copy()
    label, history, leads, converged, settled, n_iter = None, [], [], False, False, 0
    for n_iter in range(1, max_iter + 1):
        s = step(Xc, cen, label)
        history.append(s["inertia"])
        leads.append(s["lead"].min())
        if s["empty"]:
            relocate(Xc, s["new"], s["counts"], s["d2"])
        cen, label = s["new"], s["label"]
        if not s["empty"] and s["changed"] == 0:
            converged = settled = True
            break
        if not s["empty"] and s["shift2"] <= tol_abs:
            converged = True
            break
    if not settled:
        s = step(Xc, cen, label)
        leads.append(s["lead"].min())
    return dict(labels=s["label"], centroids=cen, inertia=s["inertia"], n_iter=n_iter, converged=converged,
                counts=s["counts"], history=history, min_lead=min(leads), seed_rows=rows)


def fit(X, n_clusters, seed_value=0, n_init=1, max_iter=300, tol=1e-4, round32=False):
    """The fit of mmvae_amd.clustering.kmeans_fit: rows centred on their column mean (round32: and rounded to fp32, as
    on the device), run r seeded from the r-th block of n_clusters uniforms of default_rng(seed_value), the run with the
    smallest inertia (the earlier one on ties).  The centroids come back in the caller's coordinates; `Xc` is what the
    runs saw."""
    X = np.asarray(X, dtype=np.float64)
    Xc = centred(X, round32)
    tol_abs = tol * Xc.var(0).mean()
    rng = np.random.default_rng(seed_value)
    best = None
    for _ in range(n_init):
        run = fit_run(Xc, n_clusters, rng.random(n_clusters), max_iter, tol_abs)
        if best is None or run["inertia"] < best["inertia"]:
            best = run
    best["centroids"] = best["centroids"] + X.mean(0, keepdims=True)
    best["Xc"] = Xc
    return best


# ---------------------------------------------------------------------------------------------------------- agreement
def table_of(a, b):
    """Contingency table of two code vectors; rows with a negative code are left out."""
    a, b = np.asarray(a), np.asarray(b)
    keep = (a >= 0) & (b >= 0)
    a, b = a[keep], b[keep]
    t = np.zeros((a.max() + 1 if len(a) else 0, b.max() + 1 if len(b) else 0), dtype=np.int64)
    for i, j in zip(a, b):
        t[i, j] += 1
    return t


def ari(a, b):
    """(sum_ij C(n_ij, 2) - E) / ((sum_i C(a_i, 2) + sum_j C(b_j, 2)) / 2 - E), E = sum_i C(a_i, 2) sum_j C(b_j, 2) /
    C(n, 2); 1 where the denominator vanishes (both partitions trivial in the same way)."""
    t = table_of(a, b)
    n = int(t.sum())
    pairs = lambda v: sum(math.comb(int(m), 2) for m in np.ravel(v))  # noqa: E731
    index, rows, cols, total = pairs(t), pairs(t.sum(1)), pairs(t.sum(0)), math.comb(n, 2)
    if total == 0:
        return 1.0
    expected = rows * cols / total
    top = 0.5 * (rows + cols)
    if top == expected:
        return 1.0
    return (index - expected) / (top - expected)


def nmi(a, b):
    """I(A; B) / ((H(A) + H(B)) / 2) with natural logarithms; 1 where both sides are a single class, 0 where I = 0."""
    t = table_of(a, b).astype(np.float64)
    n = t.sum()
    p = t / n
    pa, pb = p.sum(1), p.sum(0)
    if (pa > 0).sum() == 1 and (pb > 0).sum() == 1:
        return 1.0
    mi = 0.0
    for i in range(t.shape[0]):
        for j in range(t.shape[1]):
            if p[i, j] > 0:
                mi += p[i, j] * math.log(p[i, j] / (pa[i] * pb[j]))
    if mi <= 0:
        return 0.0
    h = lambda q: -sum(v * math.log(v) for v in q if v > 0)  # noqa: E731
    return mi / (0.5 * (h(pa) + h(pb)))
