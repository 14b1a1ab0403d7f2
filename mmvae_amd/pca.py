"""Principal components of latent embeddings and the principal-component regression (PCR) of covariates on them: scIB's
`pc_regression` / `pcr_comparison` (Luecken et al. 2022), the one batch-removal score that is no function of the kNN graph
and the one that takes continuous covariates (libmmvae_pca.so, include/mmvae_pca.h).

    group_sums, scatter, project   the three device entries: per-class fp64 column sums, the centred scatter, the scores
    pca_fit / pca_transform        the PCA of z [N, D <= 512]: fp64 `eigh` of the device's D x D scatter on the host
    pca_embeddings                 the first components' scores, for plots.plot_category
    pcr_from_moments               R2 per component and the variance-weighted R2Var from the moments alone (host, fp64)
    pc_regression                  the whole call on embeddings and their metadata, with a summary table
    pcr_comparison                 scIB's (pcr_pre - pcr_post) / pcr_pre
    pcr_from_predictions           stored predictions in, CSV tables out

Everything that scales with N runs in the library: one pass for the column sums, one for the scatter of [z | numeric
covariates], per categorical covariate one device sort and one class-sums pass.  What is left is D x D work in fp64.

Device tensors run the HIP kernels, always.  CPU tensors are refused outside `backend.cpu_plumbing()`; inside it every
entry is its statement in torch ops, fp64 where it sums (tests/pcr_restatement.py restates it independently).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import backend
from ._bind import ptr as _ptr, stream as _stream

MAX_D = 512
MAX_COV = 8


# ------------------------------------------------------------------------------------------------------- arguments
def _rows(x: torch.Tensor, what: str, name: str = "x") -> Tuple[torch.Tensor, int, int, int]:
    """(x, N, D, ld) of a [N, D] fp32 matrix whose rows are contiguous (a column slice of a wider one is taken as it
    is; anything else is copied)."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be fp32 [N, D], got {x.dtype} {tuple(x.shape)}")
    N, D = x.shape
    if N < 1 or D < 1:
        raise ValueError(f"{what}: {name} must have at least one row and one column, got {tuple(x.shape)}")
    if (D > 1 and x.stride(1) != 1) or (N > 1 and x.stride(0) < D):
        x = x.contiguous()
    ld = x.stride(0) if N > 1 and x.stride(0) >= D else D
    return x, N, D, ld


def _vector(v: torch.Tensor, n: int, like: torch.Tensor, what: str, name: str) -> torch.Tensor:
    if v.dtype != torch.float32 or v.shape != (n,):
        raise ValueError(f"{what}: {name} must be fp32 [{n}], got {v.dtype} {tuple(v.shape)}")
    if v.device != like.device:
        raise ValueError(f"{what}: {name} is on {v.device}, the rows on {like.device}")
    return v.contiguous()


def _pca_lib():
    from . import _pca_lib as L

    return L, L.load_pca()


# -------------------------------------------------------------------------------------------------- the three entries
def group_sums(x: torch.Tensor, order: torch.Tensor, run_ptr: torch.Tensor, mean: Optional[torch.Tensor] = None
               ) -> torch.Tensor:
    """sums [C, D] fp64: for every class c the sum of the rows order[run_ptr[c] : run_ptr[c + 1]] of x, each centred with
    ONE fp32 subtraction of `mean` (None: the raw rows).  order int32 lists rows sorted by class, run_ptr [C + 1] int32
    is non-decreasing from 0; rows that are not listed belong to no class; an empty run gives zeros."""
    x, N, D, ld = _rows(x, "group_sums")
    if D > MAX_D:
        raise ValueError(f"group_sums: at most {MAX_D} columns (got {D})")
    if order.dtype != torch.int32 or run_ptr.dtype != torch.int32 or order.dim() != 1 or run_ptr.dim() != 1:
        raise ValueError("group_sums: order and run_ptr must be int32 vectors")
    C = run_ptr.numel() - 1
    if not 1 <= C <= N or order.numel() > N:
        raise ValueError(f"group_sums: need 1 <= classes <= N and at most N listed rows (got {C} classes, "
                         f"{order.numel()} rows, N = {N})")
    if mean is not None:
        mean = _vector(mean, D, x, "group_sums", "mean")
    if not backend.on_hip(x):
        c = x if mean is None else x - mean
        counts = (run_ptr[1:] - run_ptr[:-1]).long()
        cls = torch.repeat_interleave(torch.arange(C), counts)
        out = torch.zeros((C, D), dtype=torch.float64)
        return out.index_add_(0, cls, c[order[: int(run_ptr[-1])].long()].double())
    L, lib = _pca_lib()
    order, run_ptr = order.contiguous(), run_ptr.contiguous()
    nbytes = lib.mmvae_pca_group_sums_workspace_bytes(N, D)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    out = torch.empty((C, D), dtype=torch.float64, device=x.device)
    L.check(lib.mmvae_pca_group_sums_f64(N, D, _ptr(x), ld, _ptr(mean), C, _ptr(order), _ptr(run_ptr), _ptr(out), _ptr(ws),
                                         nbytes, _stream()), "mmvae_pca_group_sums_f64")
    return out


def column_sums(x: torch.Tensor) -> torch.Tensor:
    """[D] fp64: the sums of x's columns over all rows in ascending order (one class, the identity order)."""
    N = x.shape[0]
    order = torch.arange(N, dtype=torch.int32, device=x.device)
    run_ptr = torch.tensor([0, N], dtype=torch.int32, device=x.device)
    return group_sums(x, order, run_ptr)[0]


def scatter(x: torch.Tensor, mean: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """S [W, W] fp64 with W = D + M: the scatter matrix sum_i c_i c_i^T of the centred augmented rows
    c_i = fl32([x_i | y_i] - mean), mean [W] fp32; y [N, M <= 8] fp32 holds numeric covariates (None: M = 0).  On the
    device the products of 256 consecutive rows form one exact-fp32 MFMA chain, the chains are added in fp64, and S
    is symmetric bit for bit (include/mmvae_pca.h)."""
    x, N, D, ld = _rows(x, "scatter")
    M, ldy = 0, 0
    if y is not None:
        y, Ny, M, ldy = _rows(y, "scatter", "y")
        if Ny != N or y.device != x.device:
            raise ValueError(f"scatter: y must have x's {N} rows and device, got {Ny} rows on {y.device}")
    if M > MAX_COV or D + M > MAX_D:
        raise ValueError(f"scatter: at most {MAX_COV} covariates and {MAX_D} columns in all (got D = {D}, M = {M})")
    mean = _vector(mean, D + M, x, "scatter", "mean")
    if not backend.on_hip(x):
        a = x if y is None else torch.cat([x, y], 1)
        c = (a - mean).double()
        return c.T @ c
    L, lib = _pca_lib()
    nbytes = lib.mmvae_pca_scatter_workspace_bytes(N, D, M)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    out = torch.empty((D + M, D + M), dtype=torch.float64, device=x.device)
    L.check(lib.mmvae_pca_scatter_f32(N, D, _ptr(x), ld, M, _ptr(y), ldy, _ptr(mean), _ptr(out), _ptr(ws), nbytes,
                                      _stream()), "mmvae_pca_scatter_f32")
    return out


def project(x: torch.Tensor, mean: torch.Tensor, components: torch.Tensor) -> torch.Tensor:
    """scores [N, P] fp32 = fl32(x - mean) components^T, components [P <= D, D] fp32: on the device one fp32 fmaf chain
    over the columns per score."""
    x, N, D, ld = _rows(x, "project")
    if D > MAX_D:
        raise ValueError(f"project: at most {MAX_D} columns (got {D})")
    mean = _vector(mean, D, x, "project", "mean")
    if components.dim() != 2 or components.dtype != torch.float32 or components.shape[1] != D or \
            not 1 <= components.shape[0] <= D or components.device != x.device:
        raise ValueError(f"project: components must be fp32 [P <= {D}, {D}] on {x.device}, got {components.dtype} "
                         f"{tuple(components.shape)} on {components.device}")
    P = components.shape[0]
    if not backend.on_hip(x):
        return ((x - mean).double() @ components.double().T).float()
    L, lib = _pca_lib()
    components = components.contiguous()
    out = torch.empty((N, P), dtype=torch.float32, device=x.device)
    L.check(lib.mmvae_pca_project_f32(N, D, _ptr(x), ld, _ptr(mean), P, _ptr(components), _ptr(out), P, _stream()),
            "mmvae_pca_project_f32")
    return out


# ---------------------------------------------------------------------------------------------------- the host side
def principal_axes(scatter_dd: np.ndarray, n_comps: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(eigenvalues [P], components [P, D]) of a symmetric D x D scatter matrix in fp64: `numpy.linalg.eigh`, sorted by
    descending eigenvalue, every component signed so that its entry of the largest magnitude is positive (ties: the
    smaller index) -- scikit-learn's svd_flip(u_based_decision=False)."""
    S = np.asarray(scatter_dd, dtype=np.float64)
    D = S.shape[0]
    P = D if n_comps is None else int(n_comps)
    if S.shape != (D, D) or not 1 <= P <= D:
        raise ValueError(f"principal_axes: need a square matrix and 1 <= n_comps <= {D} (got {S.shape}, {n_comps})")
    lam, vec = np.linalg.eigh(S)
    pick = np.argsort(-lam, kind="stable")[:P]
    lam, V = lam[pick], vec[:, pick].T.copy()
    big = np.argmax(np.abs(V), axis=1)
    V *= np.where(V[np.arange(P), big] < 0, -1.0, 1.0)[:, None]
    return lam, V


@dataclass
class PCAFit:
    """What `pca_fit` returns.  mean and components stay on the embeddings' device; the rest is fp64 on the host."""
    mean: torch.Tensor                    # [D] fp32: the fp64 column means rounded once
    components: torch.Tensor              # [P, D] fp32, rows of unit length, by descending eigenvalue
    explained_variance: np.ndarray        # [P] lambda / (N - 1)
    explained_variance_ratio: np.ndarray  # [P] over the KEPT components, as scIB computes Var
    scatter: np.ndarray                   # [W, W] fp64: the whole matrix of [z | covariates], W = D + M
    n_rows: int
    eigenvalues: np.ndarray               # [P] fp64, of the D x D block of `scatter`
    components64: np.ndarray              # [P, D] fp64: what `components` was rounded from
    covariate_mean: Optional[torch.Tensor] = None  # [M] fp32


def pca_fit(z: torch.Tensor, n_comps: Optional[int] = None, covariates: Optional[torch.Tensor] = None) -> PCAFit:
    """The PCA of z [N >= 2, D <= 512] fp32.  Two device passes (column sums, then the scatter of the rows centred with the
    fp32 mean), one read-back of the scatter (at most 2 MB) and `principal_axes` on the host.  `covariates` [N, M <= 8]
    fp32 are centred and multiplied in the same pass as extra columns (for `pcr_from_moments`)."""
    z, N, D, _ = _rows(z, "pca_fit", "z")
    if N < 2:
        raise ValueError("pca_fit: need at least two rows")
    mean = (column_sums(z) / N).float()
    cov_mean = None
    full = mean
    if covariates is not None:
        covariates = _rows(covariates, "pca_fit", "covariates")[0]
        cov_mean = (column_sums(covariates) / N).float()
        full = torch.cat([mean, cov_mean])
    S = scatter(z, full, covariates).cpu().numpy()
    lam, V = principal_axes(S[:D, :D], n_comps)
    total = lam.sum()
    ratio = lam / total if total > 0 else np.full_like(lam, np.nan)
    return PCAFit(mean, torch.from_numpy(V.astype(np.float32)).to(z.device), lam / (N - 1), ratio, S, N, lam, V, cov_mean)


def pca_transform(fit: PCAFit, z: torch.Tensor) -> torch.Tensor:
    """scores [N, P] fp32 of z's rows on the fit's components, on z's device."""
    return project(z, fit.mean, fit.components)


def pca_embeddings(z: torch.Tensor, n_comps: int = 2) -> torch.Tensor:
    """The scores of z on its first `n_comps` principal components: the linear picture beside `umap_embeddings`, in the
    form `plots.plot_category` takes."""
    return pca_transform(pca_fit(z, n_comps), z)


def pcr_from_moments(scatter, n_rows: int, n_comps: Optional[int] = None, class_sums=None, class_counts=None,
                     cov_index: Optional[int] = None, n_features: Optional[int] = None) -> Tuple[np.ndarray, float]:
    """(R2 per component [P], R2Var) of one covariate on the principal components, from the moments alone, in fp64.

    scatter [W, W]: the centred scatter of [z | numeric covariates]; its leading D x D block gives the components
    (`principal_axes`).  D = `n_features` (default: the columns of class_sums).
    Categorical: class_sums [C, D] holds the sums of the centred rows per class and class_counts [C] their sizes;
    R2_j = sum_c n_c (v_j . m_c)^2 / lambda_j with m_c the class mean -- what a least-squares fit of the scores on the
    class dummies with an intercept explains.  Numeric covariate cov_index = m:
    R2_j = (v_j . S[:D, D + m])^2 / (lambda_j S[D + m, D + m]).
    R2Var = sum_j lambda_j R2_j / sum_j lambda_j over the kept components (scIB's pc_regression).  A component with
    lambda_j <= 0 has R2_j = 0; a constant covariate (fewer than two classes, or no variance) gives NaN."""
    S = np.asarray(scatter, dtype=np.float64)
    if (class_sums is None) == (cov_index is None):
        raise ValueError("pcr_from_moments: give class_sums with class_counts, or cov_index")
    if n_features is None:
        if class_sums is None:
            raise ValueError("pcr_from_moments: n_features is needed with cov_index")
        n_features = np.asarray(class_sums).shape[1]
    D = int(n_features)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or not 1 <= D <= S.shape[0] or int(n_rows) < 2:
        raise ValueError(f"pcr_from_moments: need a square scatter of at least {D} columns and two rows (got {S.shape})")
    lam, V = principal_axes(S[:D, :D], n_comps)
    nan = np.full(len(lam), np.nan)
    if class_sums is not None:
        sums = np.asarray(class_sums, dtype=np.float64)
        counts = np.asarray(class_counts, dtype=np.float64)
        if sums.shape != (len(counts), D):
            raise ValueError(f"pcr_from_moments: class_sums must be [{len(counts)}, {D}], got {sums.shape}")
        filled = counts > 0
        if int(filled.sum()) < 2:
            return nan, float("nan")
        explained = (((sums[filled] @ V.T) ** 2) / counts[filled][:, None]).sum(0)
    else:
        m = D + int(cov_index)
        if not D <= m < S.shape[0]:
            raise ValueError(f"pcr_from_moments: cov_index {cov_index} outside the scatter's {S.shape[0] - D} covariates")
        if not S[m, m] > 0:
            return nan, float("nan")
        explained = (V @ S[:D, m]) ** 2 / S[m, m]
    live = lam > 0
    r2 = np.where(live, explained / np.where(live, lam, 1.0), 0.0)
    total = lam.sum()
    return r2, float((lam * r2).sum() / total) if total > 0 else float("nan")


# ------------------------------------------------------------------------------------------------------ the whole call
SUMMARY_COLUMNS = ("covariate", "kind", "n_classes", "n_cells", "n_comps", "pcr")


@dataclass
class PCRResult:
    """What `pc_regression` returns: the tables are pandas frames on the host."""
    summary: object          # one row per covariate (SUMMARY_COLUMNS)
    per_component: object    # pc, explained_variance_ratio, then one r2.{covariate} column each
    fit: PCAFit

    def pcr(self, covariate: str) -> float:
        row = self.summary[self.summary["covariate"] == covariate]
        if not len(row):
            raise KeyError(covariate)
        return float(row["pcr"].iloc[0])


def sorted_classes(codes: torch.Tensor, n_classes: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(order int32, run_ptr [n_classes + 1] int32, counts [n_classes] int64) of class codes in [0, n_classes) on the
    codes' device: a stable sort, so that a class lists its rows in ascending order."""
    order = torch.sort(codes, stable=True)[1].to(torch.int32)
    counts = torch.bincount(codes.long(), minlength=n_classes)
    run_ptr = torch.zeros(n_classes + 1, dtype=torch.int32, device=codes.device)
    run_ptr[1:] = torch.cumsum(counts, 0)
    return order, run_ptr, counts


def _is_numeric(column) -> bool:
    import pandas as pd

    return pd.api.types.is_numeric_dtype(column.dtype) and not pd.api.types.is_bool_dtype(column.dtype)


def pc_regression(z: torch.Tensor, metadata, covariates: Sequence[str] = ("species",), n_comps: Optional[int] = None
                  ) -> PCRResult:
    """scIB's principal-component regression of every metadata column in `covariates` on the PCA of z [N, D <= 512].

    A numeric column (at most 8, none missing) travels as an extra column of the one scatter pass; any other column is
    categorical: its codes come from `mixing.factorize`, the rows whose value is missing form a class of their own, and
    the column costs one device sort and one class-sums pass.  summary: one row per covariate (SUMMARY_COLUMNS; `pcr` is
    R2Var).  per_component: pc (from 1), explained_variance_ratio, and r2.{covariate}."""
    import pandas as pd

    from .mixing import factorize

    if isinstance(covariates, str):
        covariates = (covariates,)
    covariates = tuple(covariates)
    z, N, D, _ = _rows(z, "pc_regression", "z")
    missing = [c for c in covariates if c not in metadata.columns]
    if missing:
        raise KeyError(f"pc_regression: metadata has no column {missing} (it has {list(metadata.columns)})")
    if len(metadata) != N:
        raise ValueError(f"pc_regression: {N} embeddings but {len(metadata)} metadata rows")
    numeric = [c for c in covariates if _is_numeric(metadata[c])]
    if len(numeric) > MAX_COV:
        raise ValueError(f"pc_regression: at most {MAX_COV} numeric covariates in one call (got {len(numeric)})")
    y = None
    if numeric:
        values = np.ascontiguousarray(metadata[numeric].to_numpy(dtype=np.float32))
        if not np.isfinite(values).all():
            raise ValueError(f"pc_regression: the numeric covariates {numeric} must be finite in every row")
        y = torch.from_numpy(values).to(z.device)
    fit = pca_fit(z, n_comps, y)
    P = len(fit.eigenvalues)
    rows, columns = [], {"pc": np.arange(1, P + 1), "explained_variance_ratio": fit.explained_variance_ratio}
    for name in covariates:
        if name in numeric:
            r2, r2var = pcr_from_moments(fit.scatter, N, P, cov_index=numeric.index(name), n_features=D)
            rows.append((name, "numeric", 0, N, P, r2var))
        else:
            codes, uniques = factorize(metadata[name])
            L = len(uniques)
            absent = codes < 0
            if bool(absent.any()):
                codes = torch.where(absent, torch.full_like(codes, L), codes)
                L += 1
            L = max(L, 1)
            order, run_ptr, counts = sorted_classes(codes.to(z.device), L)
            sums = group_sums(z, order, run_ptr, fit.mean)
            r2, r2var = pcr_from_moments(fit.scatter, N, P, class_sums=sums.cpu().numpy(), class_counts=counts.cpu().numpy(),
                                         n_features=D)
            rows.append((name, "categorical", L, N, P, r2var))
        columns[f"r2.{name}"] = r2
    return PCRResult(pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS)), pd.DataFrame(columns), fit)


def pcr_comparison(pre: torch.Tensor, post: torch.Tensor, metadata, covariate: str, scale: bool = True,
                   n_comps: Optional[int] = None) -> float:
    """scIB's pcr_comparison: how much of the covariate's variance contribution an integration removed.  `pre` is any
    [N, D <= 512] matrix of the unintegrated cells (e.g. a user's own principal components of the expression), `post` the
    embeddings.  scale: (pcr_pre - pcr_post) / pcr_pre, and 0 when the contribution rose; otherwise the difference.
    NaN where either PCR is NaN (a constant covariate) and, scaled, where pcr_pre is 0 (nothing to remove)."""
    before = pc_regression(pre, metadata, (covariate,), n_comps).pcr(covariate)
    after = pc_regression(post, metadata, (covariate,), n_comps).pcr(covariate)
    if not scale:
        return before - after
    if math.isnan(before) or math.isnan(after) or before == 0.0:
        return float("nan")
    score = (before - after) / before
    return 0.0 if score < 0 else score


def _display(v):
    return v.decode() if isinstance(v, bytes) else v


def write_tables(result: PCRResult, save_dir: str, key: str) -> list:
    """`save_dir`/pcr.{key}.csv (the summary) and pcr.{key}.components.csv (R2 per component); the paths."""
    os.makedirs(save_dir, exist_ok=True)
    paths = [os.path.join(save_dir, f"pcr.{key}.csv"), os.path.join(save_dir, f"pcr.{key}.components.csv")]
    result.summary.to_csv(paths[0], index=False)
    result.per_component.to_csv(paths[1], index=False)
    return paths


def pcr_from_predictions(path: str, keys: Sequence[str], covariates: Sequence[str] = ("species",),
                         save_dir: Optional[str] = None, **kw) -> list:
    """`pc_regression` of stored predictions, in the two input forms of `graph_metrics.metrics_from_predictions`: a
    directory holding `{key}_embeddings.npz` with `{key}_metadata.pkl`, or a predictions.h5 read through
    `predictions.load_from_hdf5`.  Writes the tables of `write_tables` into `save_dir` (default: the directory, or the
    file's) and returns their paths."""
    from .plots import _as_points, _load_pair

    paths = []
    for key in keys:
        if path.endswith(".h5"):
            from . import predictions as P

            if not os.path.exists(path):
                raise FileNotFoundError(path)
            X, metadata, _ = P.load_from_hdf5(path, key)
            if X is None or metadata is None:
                raise KeyError(f"{path}: group {key!r} holds no embeddings with metadata")
            out_dir = save_dir or os.path.dirname(path) or "."
        else:
            X, metadata = _load_pair(os.path.join(path, f"{key}_embeddings.npz"), os.path.join(path, f"{key}_metadata.pkl"))
            out_dir = save_dir or path
        paths += write_tables(pc_regression(_as_points(X), metadata, covariates, **kw), out_dir, key)
    return paths
