"""An independent numpy restatement of include/mmvae_pca.h and of the host side of mmvae_amd/pca.py, in fp64: the centred
rows from the same fp32 inputs and fp32 mean, their scatter, class sums and projection, the PCR from those moments, and a
DIRECT form that fits every component's scores on the class dummies by least squares.  A helper module (no tests)."""
import numpy as np


# ----------------------------------------------------------------------------------------------------------- the data
def scaled_batches(seed=0, n=600, dim=12, n_batches=3, shift=1.5):
    """(X [n, dim] fp32, batch [n]): Gaussian rows whose axis d has scale 2^-d (distinct scales keep the eigen-gaps of
    the scatter wide), every batch shifted by its own vector of that same scaling.  Nothing is moved off the origin, so
    that rounding the column means to fp32 changes a column by 2^-25 of its own scale at the most."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** -np.arange(dim)
    batch = rng.integers(0, n_batches, n)
    centres = shift * rng.standard_normal((n_batches, dim))
    X = (rng.standard_normal((n, dim)) + centres[batch]) * scale
    return X.astype(np.float32), batch.astype(np.int32)


# -------------------------------------------------------------------------------------------------------- the moments
def mean32(A):
    """The fp32 mean the library's caller makes: the fp64 column sums over N, rounded once."""
    A = np.asarray(A, dtype=np.float32)
    return (A.astype(np.float64).sum(0) / len(A)).astype(np.float32)


def centred(A, mean):
    """c = fl32(a - mean) as fp64 numbers: ONE fp32 subtraction."""
    return (np.asarray(A, dtype=np.float32) - np.asarray(mean, dtype=np.float32)).astype(np.float64)


def scatter(X, mean, Y=None):
    """(S [W, W], sum_i |c_iu c_iv| [W, W]) of the augmented rows [X | Y]."""
    A = np.asarray(X, np.float32) if Y is None else np.concatenate([np.asarray(X, np.float32), np.asarray(Y, np.float32)], 1)
    c = centred(A, mean)
    return c.T @ c, np.abs(c).T @ np.abs(c)


def class_sums(X, mean, order, run_ptr):
    """(sums [C, D], sum |c| [C, D]) over the listed rows; mean None: the raw rows."""
    X = np.asarray(X, np.float32)
    c = X.astype(np.float64) if mean is None else centred(X, mean)
    C = len(run_ptr) - 1
    sums, mags = np.zeros((C, X.shape[1])), np.zeros((C, X.shape[1]))
    for k in range(C):
        rows = c[np.asarray(order[run_ptr[k]:run_ptr[k + 1]], dtype=np.int64)]
        sums[k], mags[k] = rows.sum(0), np.abs(rows).sum(0)
    return sums, mags


def projection(X, mean, components):
    """(scores [N, P], sum_d |c_id v_pd| [N, P]) with the fp32 components taken as they are."""
    c = centred(X, mean)
    V = np.asarray(components, dtype=np.float32).astype(np.float64)
    return c @ V.T, np.abs(c) @ np.abs(V).T


def runs_of(codes, n_classes):
    """(order int32, run_ptr int32 [n_classes + 1], counts) of codes in [0, n_classes); negative codes are left out."""
    codes = np.asarray(codes)
    kept = np.nonzero(codes >= 0)[0]
    order = kept[np.argsort(codes[kept], kind="stable")].astype(np.int32)
    counts = np.bincount(codes[kept], minlength=n_classes)
    run_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return order, run_ptr, counts


# ------------------------------------------------------------------------------------------------------------ the PCR
def axes(S_dd, n_comps=None):
    """(lambda [P], V [P, D]): eigh, descending, the entry of the largest magnitude of every component positive (ties:
    the smaller index)."""
    w, U = np.linalg.eigh(np.asarray(S_dd, dtype=np.float64))
    D = len(w)
    P = D if n_comps is None else n_comps
    lam, V = w[::-1][:P].copy(), U[:, ::-1][:, :P].T.copy()
    for j in range(P):
        top = 0
        for d in range(1, D):
            if abs(V[j, d]) > abs(V[j, top]):
                top = d
        if V[j, top] < 0:
            V[j] = -V[j]
    return lam, V


def from_moments(S, n_rows, n_comps=None, sums=None, counts=None, cov=None, n_features=None):
    """(R2 per component, R2Var) as include/mmvae_pca.h and pca.pcr_from_moments define them."""
    S = np.asarray(S, dtype=np.float64)
    D = n_features if n_features is not None else np.asarray(sums).shape[1]
    lam, V = axes(S[:D, :D], n_comps)
    r2 = np.zeros(len(lam))
    if sums is not None:
        sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.float64)
        if (counts > 0).sum() < 2:
            return np.full(len(lam), np.nan), float("nan")
        for j in range(len(lam)):
            got = 0.0
            for s, n in zip(sums, counts):
                if n > 0:
                    m = float(V[j] @ s) / n
                    got += n * m * m
            r2[j] = got / lam[j] if lam[j] > 0 else 0.0
    else:
        m = D + cov
        if not S[m, m] > 0:
            return np.full(len(lam), np.nan), float("nan")
        for j in range(len(lam)):
            r2[j] = float(V[j] @ S[:D, m]) ** 2 / (lam[j] * S[m, m]) if lam[j] > 0 else 0.0
    return r2, float((lam * r2).sum() / lam.sum())


def direct(X, covariate, categorical, n_comps=None):
    """(R2 per component, R2Var, lambda, V) the long way: centre with the fp32 mean, take the axes of the scatter,
    project, and fit every component's scores on [1 | design] with numpy.linalg.lstsq; R2 = 1 - SS_res / SS_tot about
    the scores' own mean, as LinearRegression.score computes it.  The design is one dummy per value (a missing value,
    code < 0, is a value of its own) or the numeric column."""
    X = np.asarray(X, np.float32)
    c = centred(X, mean32(X))
    lam, V = axes(c.T @ c, n_comps)
    scores = c @ V.T
    cov = np.asarray(covariate)
    if categorical:
        values = np.unique(cov)
        design = (cov[:, None] == values[None, :]).astype(np.float64)
    else:
        design = cov.astype(np.float32).astype(np.float64)[:, None]
    design = np.concatenate([np.ones((len(X), 1)), design], 1)
    r2 = np.zeros(len(lam))
    for j in range(len(lam)):
        t = scores[:, j]
        coef = np.linalg.lstsq(design, t, rcond=None)[0]
        res = t - design @ coef
        r2[j] = 1.0 - (res @ res) / ((t - t.mean()) @ (t - t.mean()))
    var = scores.var(0, ddof=1)
    return r2, float((var * r2).sum() / var.sum()), lam, V
