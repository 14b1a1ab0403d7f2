"""An independent numpy fp64 restatement of the definitions of include/mmvae_mix.h, written as loops over rows.  It
shares no code with mmvae_amd/mixing.py.  A helper module of tests/test_mixing_host.py and tests/test_mixing_gpu.py.

Beside every result it says how far the result can be trusted to the last bit:

    firm[i]     no |H - log perplexity| the calibration of row i visited lies within 1e-9 of tol or of 0, so two correct
                fp64 evaluations of H (another exp, another order of summation: errors near 1e-15) take the same decisions
                and -- the beta sequence being exact arithmetic -- end at the same beta after the same number of moves
    margin[i]   for the label transfer, by how much the winning mass leads the runner-up (inf with fewer than two labels)
"""
import math

import numpy as np

TOL = 1e-5
MAX_TRIES = 50
FIRM = 1e-9


# ------------------------------------------------------------------------------------------------------------ inputs
def gaussian(seed, n, dim):
    return np.random.default_rng(seed).standard_normal((n, dim))


def clusters(seed, n, dim, n_clusters=4, spread=0.15):
    """(points, cluster of every point): `n_clusters` Gaussian blobs around random unit directions."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    which = rng.integers(0, n_clusters, n)
    return centres[which] + spread * rng.standard_normal((n, dim)), which


def duplicates(seed, n, dim, group):
    """Rows of exact duplicates: consecutive runs of `group` equal rows (the last run may be shorter)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(((n + group - 1) // group, dim))
    return np.repeat(base, group, axis=0)[:n].copy()


def cosine_knn(X, k):
    """(idx [N, k] int32, dist [N, k] float32) by brute force in fp64: rows sorted by (distance, index), rank 0 the point
    itself at distance 0; the distances rounded to fp32, as the device graph stores them."""
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    norm = np.sqrt((X * X).sum(1))
    U = X / np.where(norm > 0, norm, 1.0)[:, None]
    idx = np.empty((N, k), dtype=np.int32)
    dist = np.empty((N, k), dtype=np.float32)
    for i in range(N):
        d = np.maximum(1.0 - U @ U[i], 0.0).astype(np.float32)  # rounded first: the order is that of the stored values
        d[i] = -1.0
        order = np.lexsort((np.arange(N), d))[:k]
        idx[i] = order
        dist[i] = d[order]
        dist[i, 0] = 0.0
    return idx, dist


# ------------------------------------------------------------------------------------------------------- calibration
def shifted(dist_row):
    d = dist_row.astype(np.float64)
    return d[1:] - d[1]


def weights(beta, d):
    e = np.array([math.exp(-beta * v) for v in d])
    s = 0.0
    for v in e:
        s += v
    return e / s, s


def entropy(beta, d):
    p, s = weights(beta, d)
    acc = 0.0
    for dv, pv in zip(d, p):
        acc += dv * pv
    return math.log(s) + beta * acc


def calibrate_row(d, perplexity):
    """(beta, tries, firm) of one row of shifted distances."""
    log_u = math.log(perplexity)
    beta, lo, hi = 1.0, -math.inf, math.inf
    tries, firm = 0, True
    while True:
        diff = entropy(beta, d) - log_u
        if abs(abs(diff) - TOL) <= FIRM or abs(diff) <= FIRM:
            firm = False
        if not (abs(diff) > TOL and tries < MAX_TRIES):
            return beta, tries, firm
        if diff > 0:
            lo = beta
            beta = beta * 2.0 if hi == math.inf else (beta + hi) / 2.0
        else:
            hi = beta
            beta = beta / 2.0 if lo == -math.inf else (beta + lo) / 2.0
        tries += 1


def calibrate(dist, perplexity):
    N, k = dist.shape
    assert 1.0 < perplexity < k - 1
    beta, tries, firm = np.empty(N), np.empty(N, dtype=np.int32), np.empty(N, dtype=bool)
    for i in range(N):
        beta[i], tries[i], firm[i] = calibrate_row(shifted(dist[i]), perplexity)
    return beta, tries, firm


# -------------------------------------------------------------------------------------------------------------- LISI
def lisi(idx, dist, beta, codes):
    """[N] fp64 for one code column [N] (negative = unlabelled)."""
    N, k = idx.shape
    out = np.empty(N)
    for i in range(N):
        p, _ = weights(beta[i], shifted(dist[i]))
        c = [int(codes[j]) for j in idx[i, 1:]]
        num, den = 0.0, 0.0
        for j in range(k - 1):
            if c[j] < 0:
                continue
            m = 0.0
            for l in range(k - 1):
                if c[l] >= 0 and c[l] == c[j]:
                    m += p[l]
            num += p[j] * m
            den += p[j]
        if not any(v >= 0 for v in c):
            out[i] = math.nan
            continue
        with np.errstate(all="ignore"):
            out[i] = np.float64(1.0) / (np.float64(num) / (np.float64(den) * np.float64(den)))
    return out


# ---------------------------------------------------------------------------------------------------- label transfer
def transfer(idx, dist, beta, batch, label):
    """(pred [N] int32, conf [N], cross [N], margin [N])."""
    N, k = idx.shape
    pred = np.empty(N, dtype=np.int32)
    conf, cross, margin = np.empty(N), np.empty(N), np.empty(N)
    for i in range(N):
        p, _ = weights(beta[i], shifted(dist[i]))
        mass = {}
        total = 0.0
        for rank, j in enumerate(idx[i, 1:]):
            if batch[j] >= 0 and batch[j] != batch[i] and label[j] >= 0:
                mass[int(label[j])] = mass.get(int(label[j]), 0.0) + p[rank]
                total += p[rank]
        if not mass:
            pred[i], conf[i], cross[i], margin[i] = -1, 0.0, 0.0, math.inf
            continue
        ranked = sorted(mass.items(), key=lambda kv: (-kv[1], kv[0]))
        pred[i] = ranked[0][0]
        with np.errstate(all="ignore"):
            conf[i] = np.float64(ranked[0][1]) / np.float64(total)
        cross[i] = total
        margin[i] = ranked[0][1] - ranked[1][1] if len(ranked) > 1 else math.inf
    return pred, conf, cross, margin
