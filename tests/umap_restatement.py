"""The UMAP of include/mmvae_umap.h restated in numpy / scipy, fp64 throughout: the yardstick of tests/test_umap_*.py.

Nothing here imports the project, and nothing here was fitted to the device's output: every function restates one of
umap-learn's, cited by name, with the deviations DESIGN.md lists (Jacobi updates, exactly five negatives per firing,
Philox negatives instead of tau_rand_int, no spectral init).

    cosine_knn              umap.umap_.nearest_neighbors(metric="cosine"), exact instead of NN-descent
    smooth_knn_dist         umap.umap_.smooth_knn_dist(local_connectivity=1.0, bandwidth=1.0)
    membership_strengths    umap.umap_.compute_membership_strengths
    symmetrise              the set-union step of umap.umap_.fuzzy_simplicial_set(set_op_mix_ratio=1.0)
    find_ab_params          umap.umap_.find_ab_params
    prune_and_samples       umap.umap_.simplicial_set_embedding (the `graph.data < max / n_epochs` cut) and
                            umap.layouts.make_epochs_per_sample, as whole sample counts
    layout_epoch            umap.layouts._optimize_layout_euclidean_single_epoch (with umap.layouts.clip), owner-computes
    optimize_layout         umap.layouts.optimize_layout_euclidean
"""
import numpy as np
import scipy.optimize
import scipy.sparse

from tests import philox_mirror as PM

SMOOTH_K_TOLERANCE = 1e-5
MIN_K_DIST_SCALE = 1e-3
NEGATIVE_SAMPLE_RATE = 5


# ------------------------------------------------------------------------------------------------------- 1. kNN graph
def cosine_distances(X):
    """[N, N] fp64: max(0, 1 - <x_i, x_j> / (|x_i| |x_j|)); a zero-norm row is at distance 1 from every other row."""
    X = np.asarray(X, dtype=np.float64)
    norm = np.sqrt((X * X).sum(1))
    U = np.where(norm[:, None] > 0, X / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
    return np.maximum(1.0 - U @ U.T, 0.0)


def cosine_knn(X, k):
    """(idx [N, k] int64, dist [N, k] fp64, full [N, N] fp64): rows sorted by (distance, index), rank 0 the point itself
    at distance 0 (umap-learn's n_neighbors counts the point)."""
    full = cosine_distances(X)
    N = full.shape[0]
    keyed = full.copy()
    keyed[np.arange(N), np.arange(N)] = -1.0  # the point first, whatever duplicates it has
    idx = np.argsort(keyed, axis=1, kind="stable")[:, :k]  # stable: ties in index order
    dist = np.take_along_axis(full, idx, axis=1)
    dist[:, 0] = 0.0
    return idx, dist, full


# ------------------------------------------------------------------------------------------------ 2. fuzzy simplicial set
def smooth_knn_dist(dist, n_iter=64):
    """(sigma [N], rho [N]) of umap-learn's smooth_knn_dist for local_connectivity = 1, bandwidth = 1."""
    dist = np.asarray(dist, dtype=np.float64)
    N, k = dist.shape
    target = np.log2(k)
    rho, sigma = np.zeros(N), np.zeros(N)
    mean_all = dist.mean()
    for i in range(N):
        nz = dist[i][dist[i] > 0.0]
        if nz.size:
            rho[i] = nz[0]
        lo, hi, mid = 0.0, np.inf, 1.0
        d = dist[i, 1:] - rho[i]
        for _ in range(n_iter):
            psum = np.where(d > 0, np.exp(-(np.maximum(d, 0.0) / mid)), 1.0).sum()
            if abs(psum - target) < SMOOTH_K_TOLERANCE:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        floor = MIN_K_DIST_SCALE * (dist[i].mean() if rho[i] > 0.0 else mean_all)
        sigma[i] = max(mid, floor)
    return sigma, rho


def smooth_sum(dist, rho, sigma):
    """sum_{j >= 1} exp(-max(d_ij - rho_i, 0) / sigma_i) per row, fp64: what the bisection drives to log2(k)."""
    d = np.maximum(np.asarray(dist, np.float64)[:, 1:] - np.asarray(rho, np.float64)[:, None], 0.0)
    return np.exp(-d / np.asarray(sigma, np.float64)[:, None]).sum(1)


def membership_strengths(idx, dist, rho, sigma):
    """w [N, k] fp64 of compute_membership_strengths: 0 for the point itself, 1 where d <= rho, else exp(-(d-rho)/sigma)."""
    idx = np.asarray(idx)
    d = np.asarray(dist, np.float64) - np.asarray(rho, np.float64)[:, None]
    s = np.asarray(sigma, np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((d <= 0.0) | (s == 0.0), 1.0, np.exp(-(np.maximum(d, 0.0) / np.where(s == 0.0, 1.0, s))))
    w[idx == np.arange(idx.shape[0])[:, None]] = 0.0
    return w


def symmetrise(idx, w):
    """G = P + P^T - P o P^T as (indptr int64, indices int32 sorted, data fp64), explicit zeros removed."""
    idx = np.asarray(idx)
    N, k = idx.shape
    rows = np.repeat(np.arange(N), k)
    P = scipy.sparse.csr_matrix((np.asarray(w, np.float64).ravel(), (rows, idx.ravel())), shape=(N, N))
    P.eliminate_zeros()
    T = P.T.tocsr()
    G = (P + T - P.multiply(T)).tocsr()
    G.eliminate_zeros()
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int32), G.data.astype(np.float64)


def fuzzy_simplicial_set(idx, dist):
    sigma, rho = smooth_knn_dist(dist)
    return symmetrise(idx, membership_strengths(idx, dist, rho, sigma))


# ------------------------------------------------------------------------------------------------------------ 3. layout
def find_ab_params(spread=1.0, min_dist=0.1):
    """(a, b) of umap-learn's find_ab_params: 1 / (1 + a x^(2b)) fitted to the offset exponential on linspace(0, 3 spread, 300)."""

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = scipy.optimize.curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def prune_and_samples(indptr, indices, data, n_epochs):
    """The pruned CSR (edges with w < max w / n_epochs dropped) and s_e = max(1, rint(n_epochs w_e / max w)) per slot."""
    data = np.asarray(data, np.float64)
    top = data.max()
    keep = ~(data < top / n_epochs)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))[keep]
    new_ptr = np.zeros(len(indptr), dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=len(indptr) - 1), out=new_ptr[1:])
    samples = np.maximum(1, np.rint(n_epochs * data[keep] / top)).astype(np.int32)
    return new_ptr, np.asarray(indices)[keep].astype(np.int32), samples


def active(n, samples, n_epochs):
    """Edge slots that fire in epoch n (1-based): integer arithmetic, s_e firings over the run, evenly spread."""
    s = np.asarray(samples, dtype=np.int64)
    return (n * s) // n_epochs > ((n - 1) * s) // n_epochs


def negatives(slots, n, N, seed):
    """[len(slots), 5] int64: sample t of slot e in epoch n = (word t % 4 of philox(2 e + t // 4, stream n, seed) * N) >> 32."""
    e = np.asarray(slots, dtype=np.uint64)
    w0 = np.stack(PM.philox4x32_10(e * np.uint64(2), n, seed), axis=1)
    w1 = np.stack(PM.philox4x32_10(e * np.uint64(2) + np.uint64(1), n, seed), axis=1)
    words = np.concatenate([w0, w1[:, :1]], axis=1).astype(np.uint64)
    return ((words * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def _clip(v):
    return np.clip(v, -4.0, 4.0)


def _sqdist(diff):
    d2 = diff[:, 0] * diff[:, 0]
    for c in range(1, diff.shape[1]):
        d2 = d2 + diff[:, c] * diff[:, c]
    return d2


def layout_epoch(y, indptr, indices, samples, n, n_epochs, a, b, seed, gamma=1.0, dtype=np.float64):
    """One epoch of the owner-computes layout from state y [N, C]: every vertex reads the old positions.  `dtype`
    np.float32 evaluates the same statement in single precision (the measure of what rounding alone does)."""
    y = np.asarray(y, dtype=dtype)
    N = y.shape[0]
    a, b, gamma = dtype(a), dtype(b), dtype(gamma)
    one, two = dtype(1.0), dtype(2.0)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    slots = np.nonzero(active(n, samples, n_epochs))[0]
    i, j = rows[slots], np.asarray(indices)[slots]
    total = np.zeros_like(y)
    diff = y[i] - y[j]
    d2 = _sqdist(diff)
    pos = d2 > 0
    safe = np.where(pos, d2, one)
    coeff = (-two * a * b * np.power(safe, b - one)) / (a * np.power(safe, b) + one)
    g = two * _clip(coeff[:, None] * diff).astype(dtype)
    g[~pos] = 0
    np.add.at(total, i, g)
    neg = negatives(slots, n, N, seed)
    for t in range(NEGATIVE_SAMPLE_RATE):
        o = neg[:, t]
        diff = y[i] - y[o]
        d2 = _sqdist(diff)
        pos = d2 > 0
        safe = np.where(pos, d2, one)
        coeff = (two * gamma * b) / ((dtype(0.001) + safe) * (a * np.power(safe, b) + one))
        g = _clip(coeff[:, None] * diff).astype(dtype)
        g[~pos] = 4
        g[o == i] = 0
        np.add.at(total, i, g)
    alpha = dtype(1.0 - (n - 1) / n_epochs)
    return (y + alpha * total).astype(dtype)


def optimize_layout(y0, indptr, indices, samples, n_epochs, a, b, seed, gamma=1.0, keep=()):
    """(final state, {n: state BEFORE epoch n for n in keep})."""
    y = np.asarray(y0, dtype=np.float64)
    kept = {}
    for n in range(1, n_epochs + 1):
        if n in keep:
            kept[n] = y.copy()
        y = layout_epoch(y, indptr, indices, samples, n, n_epochs, a, b, seed, gamma)
    return y, kept


def random_init(N, C, seed):
    """[N, C] fp64 uniform in +-10: element m = word m % 4 of philox(m // 4, stream 0, seed) through the 24-bit u01."""
    u = PM.u01(PM.words(N * C, seed, 0, 0)).reshape(-1)[:N * C].astype(np.float64)
    return (20.0 * u - 10.0).reshape(N, C)


def pca_init(X, C):
    """The first C principal components, scaled so that the largest coordinate is 10; each component's sign makes its
    largest loading positive."""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    _, vec = np.linalg.eigh(Xc.T @ Xc)
    V = vec[:, ::-1][:, :C]
    V = V * np.sign(V[np.abs(V).argmax(0), np.arange(C)])
    proj = Xc @ V
    return 10.0 * proj / np.abs(proj).max()


# ----------------------------------------------------------------------------------------------- the test set and scores
def clusters(seed=0, n_clusters=12, per=64, dim=32, scale=2.0):
    """(X [n_clusters * per, dim] fp32, labels): Gaussian clusters around centres of standard deviation `scale`."""
    rng = np.random.default_rng(seed)
    centres = scale * rng.standard_normal((n_clusters, dim))
    labels = np.repeat(np.arange(n_clusters), per)
    X = centres[labels] + rng.standard_normal((n_clusters * per, dim))
    return X.astype(np.float32), labels


def label_purity(Y, labels, k=15):
    """Mean fraction of a point's k nearest embedding neighbours (itself excluded) that carry its label."""
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())
