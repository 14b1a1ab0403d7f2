"""Independent restatement of include/mmvae_graph.h in numpy, written from the definitions and not from the kernels: the
connected components of a neighbour table by plain minimum-label sweeps (no pointer jumping, no forest), the component
sizes per class, and kBET in fp64 loops with math.lgamma.  tests/test_graph_metrics_host.py pins it against scipy."""
import math

import numpy as np

EPS = 2.0 ** -52
TINY = 1e-300
MAX_TERMS = 500


# ------------------------------------------------------------------------------------------------ connected components
def kept_edges(idx, codes=None):
    """(src, dst) of the listed edges that count: no self entries and, with codes, equal non-negative codes only."""
    idx = np.asarray(idx)
    N, k = idx.shape
    src = np.repeat(np.arange(N, dtype=np.int64), k)
    dst = idx.reshape(-1).astype(np.int64)
    keep = src != dst
    if codes is not None:
        codes = np.asarray(codes)
        keep &= (codes[src] >= 0) & (codes[src] == codes[dst])
    return src[keep], dst[keep]


def components(idx, codes=None):
    """root [N] int32: the smallest index of every vertex's component in the undirected union of the kept edges.  Every
    sweep gives each vertex the smallest label among itself and its neighbours, until a sweep changes nothing."""
    N = np.asarray(idx).shape[0]
    src, dst = kept_edges(idx, codes)
    label = np.arange(N, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, src, label[dst])
        np.minimum.at(new, dst, label[src])
        if np.array_equal(new, label):
            return label.astype(np.int32)
        label = new


def component_sizes(root, codes, n_classes):
    """(class_count [n_classes] int64, class_largest [n_classes] int32, n_components) over the labelled vertices."""
    root = np.asarray(root)
    N = len(root)
    codes = np.zeros(N, dtype=np.int32) if codes is None else np.asarray(codes)
    labelled = codes >= 0
    count = np.bincount(codes[labelled], minlength=n_classes).astype(np.int64)
    size = np.bincount(root[labelled], minlength=N)
    largest = np.zeros(n_classes, dtype=np.int32)
    is_root = labelled & (root == np.arange(N))
    np.maximum.at(largest, codes[is_root], size[is_root].astype(np.int32))
    return count, largest, int(is_root.sum())


def connectivity(idx, codes, n_classes):
    """(per class largest / count with NaN for an empty class, their mean over the non-empty classes, n_components)."""
    root = components(idx, codes)
    count, largest, n_comp = component_sizes(root, codes, n_classes)
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(count > 0, largest / np.maximum(count, 1), np.nan)
    return per, float(np.nanmean(per)) if (count > 0).any() else math.nan, n_comp


# ---------------------------------------------------------------------------------------------------------------- kBET
def gamma_q(a, x):
    """Q(a, x), the regularised upper incomplete gamma function, for x > 0."""
    front = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        ap, d = a, 1.0 / a
        s = d
        for _ in range(MAX_TERMS):
            ap += 1.0
            d *= x / ap
            s += d
            if abs(d) < abs(s) * EPS:
                break
        return 1.0 - s * front
    b = x + 1.0 - a
    c = 1.0 / TINY
    d = 1.0 / b
    h = d
    for n in range(1, MAX_TERMS + 1):
        an = -n * (n - a)
        b += 2.0
        d = an * d + b
        if abs(d) < TINY:
            d = TINY
        c = b + an / c
        if abs(c) < TINY:
            c = TINY
        d = 1.0 / d
        step = d * c
        h *= step
        if abs(step - 1.0) < EPS:
            break
    return front * h


def batch_frequencies(batch, n_batches):
    batch = np.asarray(batch)
    count = np.bincount(batch[batch >= 0], minlength=n_batches).astype(np.float64)
    return count / count.sum()


def kbet(idx, batch, n_batches, freq=None):
    """(stat [N], pval [N]) fp64: ranks 1 .. k - 1 of every row against the expected composition `freq` (default: the
    labelled cells' global frequencies); dof = the batches with freq > 0, minus 1."""
    idx, batch = np.asarray(idx), np.asarray(batch)
    N, k = idx.shape
    freq = batch_frequencies(batch, n_batches) if freq is None else np.asarray(freq, dtype=np.float64)
    dof = int((freq > 0).sum()) - 1
    a = 0.5 * dof
    stat, pval = np.empty(N), np.empty(N)
    for i in range(N):
        codes = [int(batch[j]) for j in idx[i, 1:]]
        n = [0] * n_batches
        for c in codes:
            if 0 <= c < n_batches:
                n[c] += 1
        k_i = sum(n)
        if k_i == 0:
            stat[i] = pval[i] = math.nan
            continue
        s = 0.0
        for b in range(n_batches):
            f = float(freq[b])
            if f > 0.0:
                e = float(k_i) * f
                d = float(n[b]) - e
                s += (d * d) / e
        stat[i] = s
        pval[i] = 1.0 if s == 0.0 else gamma_q(a, 0.5 * s)
    return stat, pval


def rejection_rate(pval, alpha=0.05):
    ok = ~np.isnan(pval)
    return float((pval[ok] < alpha).mean()) if ok.any() else math.nan


def kbet_k0(batch_in_class, n_batches):
    """scIB's neighbourhood size of one label class (capped at 63 neighbours): a quarter of the mean batch size, at least
    10, at most n - 2."""
    b = np.asarray(batch_in_class)
    counts = np.bincount(b[b >= 0], minlength=n_batches)
    present = counts[counts > 0]
    return int(min(63, max(10, int(math.floor(present.mean() / 4.0))), len(b) - 2))


# ---------------------------------------------------------------------------------------------------------- test inputs
def mixture(seed, n, dim, n_classes, spread=1.0, scale=2.0):
    """(points [n, dim] fp32, class of every point): Gaussian blobs around random centres."""
    rng = np.random.default_rng(seed)
    centres = scale * rng.standard_normal((n_classes, dim))
    which = rng.integers(0, n_classes, n)
    return (centres[which] + spread * rng.standard_normal((n, dim))).astype(np.float32), which.astype(np.int32)


def with_gaps(seed, codes, share):
    """A copy of `codes` with about `share` of the entries set to -1."""
    out = np.array(codes, dtype=np.int32)
    out[np.random.default_rng(seed).random(len(out)) < share] = -1
    return out


def path_table(n, order=None):
    """[n, 2] table of a path through `order` (default 0, 1, .. n - 1): every vertex lists its successor, the last one
    itself; column 0 is the vertex."""
    order = np.arange(n) if order is None else np.asarray(order)
    idx = np.empty((n, 2), dtype=np.int32)
    idx[:, 0] = np.arange(n)
    idx[order[:-1], 1] = order[1:]
    idx[order[-1], 1] = order[-1]
    return idx


def cliques_table(joined=True):
    """Two 32-cliques (vertices 0 .. 31 and 32 .. 63, every vertex listing its whole clique, itself included); with
    `joined`, vertex 31 lists vertex 32 in place of itself: the one edge between them."""
    idx = np.empty((64, 32), dtype=np.int32)
    idx[:32] = np.arange(32)
    idx[32:] = np.arange(32, 64)
    if joined:
        idx[31, 31] = 32
    return idx


def hand_tables(n_path=4096):
    """name -> (idx, codes or None, n_classes) of the hand-made component cases."""
    rng = np.random.default_rng(7)
    out = {"path": (path_table(n_path), None, 1),
           "path permuted": (path_table(n_path, rng.permutation(n_path)), None, 1)}
    ring = np.stack([np.arange(600), (np.arange(600) + 1) % 600], 1).astype(np.int32)
    out["ring"] = (ring, None, 1)
    star = np.stack([np.arange(300), np.zeros(300, dtype=np.int64)], 1).astype(np.int32)  # the hub 0 lists nobody
    out["star"] = (star, None, 1)
    out["all self"] = (np.repeat(np.arange(130, dtype=np.int32)[:, None], 3, 1), None, 1)
    out["one vertex"] = (np.zeros((1, 1), dtype=np.int32), None, 1)
    out["257 x 3"] = (rng.integers(0, 257, (257, 3)).astype(np.int32), with_gaps(8, rng.integers(0, 2, 257), 0.05), 2)
    # duplicates and self entries at non-zero ranks: pairs (2 m, 2 m + 1) and every tenth pair tied to the next one
    m = np.arange(100)
    partner = m ^ 1
    far = np.where(m % 20 == 0, (m + 2) % 100, m)
    out["duplicates and selves"] = (np.stack([partner, m, partner, far, m, far], 1).astype(np.int32), None, 1)
    same = np.zeros(64, dtype=np.int32)
    other = np.repeat(np.array([0, 1], dtype=np.int32), 32)
    gap = same.copy()
    gap[32] = -1
    out["cliques, one code"] = (cliques_table(), same, 1)
    out["cliques, two codes"] = (cliques_table(), other, 2)
    out["cliques, one end unlabelled"] = (cliques_table(), gap, 1)
    out["cliques, no codes"] = (cliques_table(), None, 1)
    return out


def knn_component_case(n, dim, k, n_classes, scale=2.0, seed=3):
    """(idx, codes with 3 % gaps, n_classes): the cosine kNN graph of a seeded Gaussian mixture, its blobs the classes;
    the smaller `scale`, the more the blobs overlap and the more cells lose touch with their class."""
    from tests.mix_restatement import cosine_knn

    X, which = mixture(seed + n, n, dim, n_classes, scale=scale)
    return cosine_knn(X, k)[0], with_gaps(seed, which, 0.03), n_classes


def random_table(n, k, seed=5):
    return np.random.default_rng(seed).integers(0, n, (n, k)).astype(np.int32)


def kbet_case(n, dim, k, n_batches, seed=9, shift=0.6):
    """(idx, batch with 2 % gaps): the cosine kNN graph of four blobs whose cells are moved by a batch-specific shift;
    the batch proportions are unequal (b + 1 parts for batch b)."""
    from tests.mix_restatement import cosine_knn

    rng = np.random.default_rng(seed + n)
    X, _ = mixture(seed + n + 1, n, dim, 4)
    share = np.arange(1, n_batches + 1, dtype=np.float64)
    batch = rng.choice(n_batches, size=n, p=share / share.sum()).astype(np.int32)
    X = X + shift * rng.standard_normal((n_batches, dim))[batch]
    return cosine_knn(X, k)[0], with_gaps(seed, batch, 0.02)


def kbet_hand_cases():
    """name -> (idx, batch, freq or None, n_batches) of the hand-made kBET rows."""
    out = {}
    # 9 cells, k = 5: cells 0 .. 3 batch 0, 4 .. 7 batch 1, cell 8 unlabelled
    batch = np.array([0, 0, 0, 0, 1, 1, 1, 1, -1], dtype=np.int32)
    idx = np.array([[0, 1, 2, 3, 0],      # every neighbour from batch 0
                    [1, 0, 2, 4, 5],      # two and two: exactly at expectation (freq 1/2, 1/2)
                    [2, 8, 8, 8, 8],      # every neighbour unlabelled
                    [3, 4, 5, 6, 7],      # every neighbour from batch 1
                    [4, 0, 8, 5, 8],      # two neighbours unlabelled: k_i = 2
                    [5, 1, 2, 3, 6], [6, 7, 4, 5, 0], [7, 8, 0, 1, 4], [8, 0, 4, 1, 5]], dtype=np.int32)
    out["two batches"] = (idx, batch, None, 2)
    out["a batch of share 0"] = (idx, batch, np.array([0.25, 0.75, 0.0]), 3)
    out["k = 2"] = (idx[:, :2].copy(), batch, None, 2)
    rng = np.random.default_rng(4)
    many = rng.integers(0, 64, 500).astype(np.int32)
    many[:64] = np.arange(64)
    # 70 cells, k = 64, five of them in a batch expected once in a million: statistics of 1e5 and more, p below 1e-290
    rare = np.zeros(70, dtype=np.int32)
    rare[::14] = 1
    ranks = (np.arange(70)[:, None] + np.arange(64)[None, :]) % 70
    out["a rare batch"] = (ranks.astype(np.int32), rare, np.array([1.0 - 1e-6, 1e-6]), 2)
    out["64 batches"] = (rng.integers(0, 500, (500, 64)).astype(np.int32), many, None, 64)
    return out
