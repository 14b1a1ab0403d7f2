"""Host-side checks of the PCA moments and the principal-component regression (no GPU): the C-ABI surface of
libmmvae_pca.so and its argument checks, `pca.pcr_from_moments` against the restatement's direct least-squares form
(tests/pcr_restatement.py) and against scikit-learn, the CPU-plumbing path of mmvae_amd.pca, the CSV writers, the
command-line tool and the Trainer's gathering.

Bounds.  The data are 600 x 12 rows in 3 batches with shifted means and per-axis scales 2^0 .. 2^-11: the eigenvalues of
the scatter fall by a factor near 4 from one to the next (the batch shifts move them; the closest pair of this seed is
0.040 and 0.032, a relative gap of 0.2), so an eigenvector moves by about 5 x 2^-52 per unit of relative perturbation
and R2 (a ratio of quadratic forms in it) agrees between two fp64 computations far inside 1e-9.
The moments form takes SS_tot about zero and the direct form about the scores' mean; the centred scores' mean is the
fp32 rounding of the column means, and a column's mean is of the size of the column's own scale (the data are not moved
off the origin), so it is at most 2^-25 * 4 of the column's standard deviation: a relative (2^-23)^2 = 1.4e-14 in
SS_tot, and as little in the rotation of the axes.  FP64_AGREE = 1e-9 holds both.

scikit-learn is given the rows every side works on: c = fl32(x - mean), ONE fp32 subtraction (include/mmvae_pca.h), as
fp64 numbers.  Given x itself it would centre in fp64, and the 2^-24 roundings of the subtraction -- a property of the
definition, not an error of either side -- move R2 by about 1e-8."""
import importlib.util
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import pcr_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_pca.h")
FP64_AGREE = 1e-9


def _close(got, want, tol=FP64_AGREE):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))).all())


def _moments(X, codes=None, n_classes=None, Y=None):
    mean = R.mean32(X)
    full = mean if Y is None else np.concatenate([mean, R.mean32(Y)])
    S, _ = R.scatter(X, full, Y)
    if codes is None:
        return S, None, None
    order, run_ptr, counts = R.runs_of(codes, n_classes)
    sums, _ = R.class_sums(X, mean, order, run_ptr)
    return S, sums, counts


# ------------------------------------------------------------------------------------------------------- the C surface
def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _bind, _pca_lib

    declared = check_surface(_pca_lib.BINDING)
    assert set(declared) == {"mmvae_pca_abi_version", "mmvae_pca_build_arch", "mmvae_pca_group_sums_workspace_bytes",
                             "mmvae_pca_group_sums_f64", "mmvae_pca_scatter_workspace_bytes", "mmvae_pca_scatter_f32",
                             "mmvae_pca_project_f32"} == set(_pca_lib.PCA_PROTOTYPES)
    assert "_pca_lib" in _bind.MORE_DEVICE_LIBRARY_MODULES and "_pca_lib" not in _bind.DEVICE_LIBRARY_MODULES


def test_versions_and_constants():
    from mmvae_amd import _clust_lib, _graph_lib, _lib, _pca_lib, pca

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _pca_lib.load_pca()
    assert define("MMVAE_PCA_ABI_VERSION") == 1 == lib.mmvae_pca_abi_version() == _pca_lib.PCA_ABI_VERSION
    assert lib.mmvae_pca_build_arch() == b"gfx950"
    assert define("MMVAE_PCA_CHAIN") == _pca_lib.PCA_CHAIN <= 1024
    assert define("MMVAE_PCA_SEGMENT") == _pca_lib.PCA_SEGMENT
    assert define("MMVAE_PCA_MAX_D") == _pca_lib.PCA_MAX_D == pca.MAX_D == 512
    assert define("MMVAE_PCA_MAX_COV") == _pca_lib.PCA_MAX_COV == pca.MAX_COV == 8
    assert define("MMVAE_PCA_PARTIAL_CAP") == _pca_lib.PCA_PARTIAL_CAP
    assert define("MMVAE_PCA_MAX_SUMS") == _pca_lib.PCA_MAX_SUMS == 2 ** 30
    # none of the new names leaked into another library's table
    for binding in (_clust_lib.BINDING, _graph_lib.BINDING):
        assert not [n for n in binding.prototypes if n.startswith("mmvae_pca_")]
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_pca_")]


def test_workspace_sizes_follow_the_shape():
    from mmvae_amd import _pca_lib

    lib = _pca_lib.load_pca()
    chain, seg, tile = _pca_lib.PCA_CHAIN, _pca_lib.PCA_SEGMENT, 64 * 64 * 8
    # one tile per (upper-triangular tile, row range); a range holds two chains where there are two
    assert lib.mmvae_pca_scatter_workspace_bytes(5, 3, 0) == tile
    assert lib.mmvae_pca_scatter_workspace_bytes(4 * chain + 37, 16, 0) == 3 * tile
    assert lib.mmvae_pca_scatter_workspace_bytes(2100, 128, 3) == 6 * 5 * tile
    assert lib.mmvae_pca_scatter_workspace_bytes(600, 504, 8) == 36 * 2 * tile
    for N in (10 ** 6, 10 ** 7, 2 ** 31 - 1):
        for D, M in ((50, 0), (128, 3), (512, 0)):
            got = lib.mmvae_pca_scatter_workspace_bytes(N, D, M)
            assert 0 < got <= _pca_lib.PCA_PARTIAL_CAP and got % 16 == 0, (N, D, M)
    assert lib.mmvae_pca_group_sums_workspace_bytes(5, 3) == 2 * 3 * 8
    assert lib.mmvae_pca_group_sums_workspace_bytes(seg + 1, 7) == 2 * 2 * 7 * 8
    for bad in ((0, 3, 0), (5, 0, 0), (5, 513, 0), (5, 505, 8), (5, 3, 9), (5, 3, -1)):
        assert lib.mmvae_pca_scatter_workspace_bytes(*bad) == 0, bad
    for bad in ((0, 3), (5, 0), (5, 513)):
        assert lib.mmvae_pca_group_sums_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below carries the fake device address 16: had one of them launched, it would not return ERR_ARG."""
    from mmvae_amd import _pca_lib

    lib = _pca_lib.load_pca()
    big = 1 << 30
    #      N   D   x  ldx mean C order run_ptr sums ws bytes stream
    ok = (100, 8, 16, 8, 16, 3, 16, 16, 16, 16, big, None)
    bad = {"N 0": {0: 0}, "D 0": {1: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: 7}, "C 0": {5: 0}, "C > N": {5: 101},
           "short workspace": {10: 15}, "odd workspace": {9: 24},
           "C D past 2^30": {0: 2 ** 31 - 1, 1: 512, 3: 512, 5: 2 ** 21 + 1, 10: 1 << 40}}
    bad.update({f"null argument {i}": {i: None} for i in (2, 6, 7, 8, 9)})
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_pca_group_sums_f64(*args) == _pca_lib.ERR_ARG, what
    #       N   D   x  ldx M  y  ldy mean out ws bytes stream
    oks = (100, 8, 16, 8, 2, 16, 2, 16, 16, 16, big, None)
    bads = {"N 0": {0: 0}, "D 0": {1: 0}, "W 513": {1: 511, 3: 511}, "D 513": {1: 513, 3: 513, 4: 0}, "ldx < D": {3: 7},
            "M 9": {4: 9, 6: 9}, "M < 0": {4: -1}, "ldy < M": {6: 1}, "null y with M": {5: None},
            "short workspace": {10: 64 * 64 * 8 - 1}, "odd workspace": {9: 8}}
    bads.update({f"null argument {i}": {i: None} for i in (2, 7, 8, 9)})
    for what, change in bads.items():
        args = [change.get(i, a) for i, a in enumerate(oks)]
        assert lib.mmvae_pca_scatter_f32(*args) == _pca_lib.ERR_ARG, what
    #       N   D   x  ldx mean P comp scores lds stream
    okp = (100, 8, 16, 8, 16, 2, 16, 16, 2, None)
    badp = {"N 0": {0: 0}, "D 0": {1: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: 7}, "P 0": {5: 0}, "P > D": {5: 9, 8: 9},
            "lds < P": {8: 1}}
    badp.update({f"null argument {i}": {i: None} for i in (2, 4, 6, 7)})
    for what, change in badp.items():
        args = [change.get(i, a) for i, a in enumerate(okp)]
        assert lib.mmvae_pca_project_f32(*args) == _pca_lib.ERR_ARG, what


# ------------------------------------------------------------------------------------- the moments against least squares
def test_restatement_and_sklearn_agree():
    """The yardstick itself: the restatement's direct form against PCA(svd_solver="full") + LinearRegression."""
    decomposition = pytest.importorskip("sklearn.decomposition")
    linear_model = pytest.importorskip("sklearn.linear_model")
    X, batch = R.scaled_batches()
    r2, r2var, lam, V = R.direct(X, batch, True)
    rows = R.centred(X, R.mean32(X))
    pca = decomposition.PCA(svd_solver="full").fit(rows)
    assert _close(pca.explained_variance_, lam / (len(X) - 1)) and _close(np.abs(pca.components_), np.abs(V), 1e-7)
    scores = pca.transform(rows)
    dummies = pd.get_dummies(batch).to_numpy(dtype=np.float64)
    want = [linear_model.LinearRegression().fit(dummies, s).score(dummies, s) for s in scores.T]
    assert _close(r2, want)
    var = scores.var(0, ddof=1)
    assert _close(r2var, (var * want).sum() / var.sum())


def test_pcr_from_moments_equals_least_squares():
    from mmvae_amd import pca

    X, batch = R.scaled_batches()
    rng = np.random.default_rng(4)
    N, D = X.shape
    # categorical
    S, sums, counts = _moments(X, batch, 3)
    r2, r2var = pca.pcr_from_moments(S, N, None, class_sums=sums, class_counts=counts)
    want = R.direct(X, batch, True)
    assert _close(r2, want[0]) and _close(r2var, want[1]) and 0.05 < r2var < 0.95
    assert _close(r2, R.from_moments(S, N, None, sums, counts)[0], 1e-12)
    # categorical with missing values: a class of their own
    holes = batch.copy()
    holes[rng.random(N) < 0.1] = -1
    codes = np.where(holes < 0, 3, holes)
    S, sums, counts = _moments(X, codes, 4)
    r2, r2var = pca.pcr_from_moments(S, N, None, class_sums=sums, class_counts=counts)
    want = R.direct(X, holes, True)
    assert _close(r2, want[0]) and _close(r2var, want[1])
    # an empty class changes nothing
    again = pca.pcr_from_moments(S, N, None, class_sums=np.vstack([sums, np.zeros(D)]), class_counts=np.append(counts, 0))
    assert np.array_equal(again[0], r2) and again[1] == r2var
    # numeric, one of two covariates
    y = np.stack([rng.standard_normal(N), X[:, 0] * 0.5 + 0.3 * rng.standard_normal(N)], 1).astype(np.float32)
    S, _, _ = _moments(X, Y=y)
    for m in (0, 1):
        r2, r2var = pca.pcr_from_moments(S, N, None, cov_index=m, n_features=D)
        want = R.direct(X, y[:, m], False)
        assert _close(r2, want[0]) and _close(r2var, want[1]), m
    assert r2[0] > 0.5  # (the second covariate follows the first axis)
    # fewer components than columns: the ratio is over the kept ones
    S, sums, counts = _moments(X, batch, 3)
    r2, r2var = pca.pcr_from_moments(S, N, 4, class_sums=sums, class_counts=counts)
    want = R.direct(X, batch, True, 4)
    assert len(r2) == 4 and _close(r2, want[0]) and _close(r2var, want[1])
    with pytest.raises(ValueError, match="n_features"):
        pca.pcr_from_moments(S, N, None, cov_index=0)
    with pytest.raises(ValueError, match="class_sums"):
        pca.pcr_from_moments(S, N, None)


def test_pcr_against_sklearn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    linear_model = pytest.importorskip("sklearn.linear_model")
    from mmvae_amd import pca

    X, batch = R.scaled_batches()
    N = len(X)
    S, sums, counts = _moments(X, batch, 3)
    r2, r2var = pca.pcr_from_moments(S, N, None, class_sums=sums, class_counts=counts)
    rows = R.centred(X, R.mean32(X))
    fit = decomposition.PCA(svd_solver="full").fit(rows)
    scores = fit.transform(rows)
    dummies = pd.get_dummies(batch).to_numpy(dtype=np.float64)
    want = np.array([linear_model.LinearRegression().fit(dummies, s).score(dummies, s) for s in scores.T])
    assert _close(r2, want) and _close(r2var, (fit.explained_variance_ * want).sum() / fit.explained_variance_.sum())


def test_constant_covariates_and_dead_components():
    from mmvae_amd import pca

    X, batch = R.scaled_batches()
    N, D = X.shape
    S, sums, counts = _moments(X, np.zeros(N, np.int32), 1)
    r2, r2var = pca.pcr_from_moments(S, N, None, class_sums=sums, class_counts=counts)
    assert np.isnan(r2).all() and len(r2) == D and math.isnan(r2var)
    S, _, _ = _moments(X, Y=np.full((N, 1), 0.1, np.float32))
    assert S[D, D] == 0.0
    r2, r2var = pca.pcr_from_moments(S, N, 3, cov_index=0, n_features=D)
    assert np.isnan(r2).all() and len(r2) == 3 and math.isnan(r2var)
    # a component with lambda = 0 has R2 = 0, whatever the class sums say
    r2, r2var = pca.pcr_from_moments(np.diag([2.0, 0.0, 1.0]), 4, None, class_sums=[[1.0, 1.0, 0.0], [-1.0, -1.0, 0.0]],
                                     class_counts=[2, 2])
    assert r2.tolist() == [0.5, 0.0, 0.0] and r2var == 1.0 / 3.0
    # a column that never varies adds a dead component and changes nothing else
    flat = X.copy()
    flat[:, 5] = 1.25
    S, sums, counts = _moments(flat, batch, 3)
    assert S[5, 5] == 0.0 and not S[5].any()
    r2, r2var = pca.pcr_from_moments(S, N, None, class_sums=sums, class_counts=counts)
    want = R.direct(np.delete(flat, 5, 1), batch, True)
    assert np.isfinite(r2).all() and _close(r2[:-1], want[0]) and _close(r2var, want[1])


def test_the_sign_rule():
    from mmvae_amd import pca

    S = np.diag([1.0, 4.0, 2.0])
    lam, V = pca.principal_axes(S)
    assert lam.tolist() == [4.0, 2.0, 1.0] and np.array_equal(V, np.eye(3)[[1, 2, 0]])
    lam, V = pca.principal_axes(np.array([[2.0, -1.0], [-1.0, 2.0]]))
    assert np.allclose(lam, [3.0, 1.0]) and V[0, 0] * V[0, 1] < 0 and V[1, 0] > 0 and V[1, 1] > 0
    assert V[0, np.abs(V[0]).argmax()] > 0  # (numpy's argmax: of equal magnitudes the smaller index)
    X, _ = R.scaled_batches()
    S, _ = R.scatter(X, R.mean32(X))
    lam, V = pca.principal_axes(S, 5)
    want_lam, want_V = R.axes(S, 5)
    assert np.array_equal(lam, want_lam) and np.array_equal(V, want_V)
    assert (V[np.arange(5), np.abs(V).argmax(1)] > 0).all() and (np.diff(lam) < 0).all()
    with pytest.raises(ValueError, match="n_comps"):
        pca.principal_axes(S, 13)


# ---------------------------------------------------------------------------------------------------- the python layer
def test_cpu_entries_equal_the_restatement():
    from mmvae_amd import backend, pca

    X, batch = R.scaled_batches(n=300, dim=7)
    y = np.random.default_rng(1).standard_normal((300, 2)).astype(np.float32)
    mean = R.mean32(X)
    full = np.concatenate([mean, R.mean32(y)])
    codes = batch.copy()
    codes[::7] = -1
    order, run_ptr, counts = R.runs_of(codes, 4)  # (class 3 is empty; a seventh of the rows is in no class)
    tx, ty = torch.from_numpy(X), torch.from_numpy(y)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        pca.scatter(tx, torch.from_numpy(mean))
    with backend.cpu_plumbing():
        S = pca.scatter(tx, torch.from_numpy(full), ty)
        sums = pca.group_sums(tx, torch.from_numpy(order), torch.from_numpy(run_ptr), torch.from_numpy(mean))
        raw = pca.column_sums(tx)
        fit = pca.pca_fit(tx, 3, ty)
        scores = pca.pca_transform(fit, tx)
        two = pca.pca_embeddings(tx)
        padded = torch.full((300, 12), float("nan"))
        padded[:, :7] = tx
        assert torch.allclose(pca.scatter(padded[:, :7], torch.from_numpy(mean)), pca.scatter(tx, torch.from_numpy(mean)),
                              rtol=1e-13, atol=0)
        with pytest.raises(ValueError, match="fp32"):
            pca.scatter(tx.double(), torch.from_numpy(mean))
        with pytest.raises(ValueError, match=r"mean must be fp32 \[9\]"):
            pca.scatter(tx, torch.from_numpy(mean), ty)
        with pytest.raises(ValueError, match="covariates"):
            pca.scatter(tx, torch.zeros(16), torch.zeros((300, 9)))
        with pytest.raises(ValueError, match="components"):
            pca.project(tx, torch.from_numpy(mean), torch.zeros((8, 7)))
        with pytest.raises(ValueError, match="int32"):
            pca.group_sums(tx, torch.from_numpy(order).long(), torch.from_numpy(run_ptr))
    assert S.dtype == sums.dtype == torch.float64 and scores.dtype == torch.float32
    assert _close(S.numpy(), R.scatter(X, full, y)[0], 1e-12) and _close(sums.numpy(), R.class_sums(X, mean, order, run_ptr)[0], 1e-12)
    assert not sums[3].any() and _close(raw.numpy(), X.astype(np.float64).sum(0), 1e-12)
    assert np.array_equal(fit.mean.numpy(), mean) and np.array_equal(fit.covariate_mean.numpy(), full[7:])
    lam, V = R.axes(fit.scatter[:7, :7], 3)
    assert fit.n_rows == 300 and fit.scatter.shape == (9, 9) and fit.components.shape == (3, 7)
    assert np.array_equal(fit.eigenvalues, lam) and np.array_equal(fit.components.numpy(), V.astype(np.float32))
    assert _close(fit.explained_variance, lam / 299, 1e-15) and _close(fit.explained_variance_ratio, lam / lam.sum(), 1e-15)
    assert _close(scores.numpy(), R.projection(X, mean, fit.components.numpy())[0], 1e-6)
    assert two.shape == (300, 2) and _close(two.numpy(), scores.numpy()[:, :2], 1e-6)


def _frame(X, batch, seed=3):
    rng = np.random.default_rng(seed)
    species = np.array(["human", "mouse", "rat"], dtype=object)[batch]
    donor = np.array([f"d{i % 5}" for i in range(len(X))], dtype=object)
    donor[rng.random(len(X)) < 0.08] = np.nan
    return pd.DataFrame({"species": species, "donor": donor, "total_counts": (40.0 * X[:, 0] + rng.standard_normal(len(X))),
                         "noise": rng.standard_normal(len(X)).astype(np.float32), "one": ["same"] * len(X)})


def test_pc_regression_on_cpu_plumbing():
    from mmvae_amd import backend, pca

    X, batch = R.scaled_batches()
    meta = _frame(X, batch)
    covariates = ("species", "total_counts", "donor", "noise", "one")
    with backend.cpu_plumbing():
        out = pca.pc_regression(torch.from_numpy(X), meta, covariates)
        few = pca.pc_regression(torch.from_numpy(X), meta, "species", n_comps=4)
        with pytest.raises(KeyError, match="tissue"):
            pca.pc_regression(torch.from_numpy(X), meta, ("tissue",))
        with pytest.raises(ValueError, match="metadata rows"):
            pca.pc_regression(torch.from_numpy(X), meta.iloc[:-1], ("species",))
        with pytest.raises(ValueError, match="finite"):
            pca.pc_regression(torch.from_numpy(X), meta.assign(noise=np.where(np.arange(600) == 5, np.nan, 1.0)), ("noise",))
    assert tuple(out.summary.columns) == pca.SUMMARY_COLUMNS and out.summary["covariate"].tolist() == list(covariates)
    assert out.summary["kind"].tolist() == ["categorical", "numeric", "categorical", "numeric", "categorical"]
    assert out.summary["n_classes"].tolist() == [3, 0, 6, 0, 1] and out.summary["n_cells"].tolist() == [600] * 5
    assert out.summary["n_comps"].tolist() == [12] * 5
    assert list(out.per_component.columns) == ["pc", "explained_variance_ratio"] + [f"r2.{c}" for c in covariates]
    assert out.per_component["pc"].tolist() == list(range(1, 13))
    assert out.fit.scatter.shape == (14, 14)
    # against least squares, covariate by covariate
    donor_codes = pd.factorize(meta["donor"], sort=True)[0]
    cases = {"species": (batch, True), "donor": (donor_codes, True),
             "total_counts": (meta["total_counts"].to_numpy(np.float32), False), "noise": (meta["noise"].to_numpy(), False)}
    for name, (cov, categorical) in cases.items():
        r2, r2var, _, _ = R.direct(X, cov, categorical)
        assert _close(out.per_component[f"r2.{name}"], r2) and _close(out.pcr(name), r2var), name
    assert out.pcr("total_counts") > 0.5 and 0.05 < out.pcr("species") < 0.95 and out.pcr("noise") < 0.05
    assert math.isnan(out.pcr("one")) and out.per_component["r2.one"].isna().all()
    assert few.summary["n_comps"].tolist() == [4] and len(few.per_component) == 4
    assert _close(few.pcr("species"), R.direct(X, batch, True, 4)[1])
    assert _close(few.per_component["explained_variance_ratio"].sum(), 1.0, 1e-14)
    with pytest.raises(KeyError):
        out.pcr("absent")


def test_pcr_comparison_scales_and_clips():
    from mmvae_amd import backend, pca

    X, batch = R.scaled_batches()
    meta = _frame(X, batch)
    rng = np.random.default_rng(8)
    mixed = (rng.standard_normal(X.shape) * 2.0 ** -np.arange(12)).astype(np.float32)  # no batch effect left
    before, after = R.direct(X, batch, True)[1], R.direct(mixed, batch, True)[1]
    assert after < 0.02 < before
    with backend.cpu_plumbing():
        t_pre, t_post = torch.from_numpy(X), torch.from_numpy(mixed)
        assert _close(pca.pcr_comparison(t_pre, t_post, meta, "species"), (before - after) / before)
        assert _close(pca.pcr_comparison(t_pre, t_post, meta, "species", scale=False), before - after)
        assert pca.pcr_comparison(t_post, t_pre, meta, "species") == 0.0  # the contribution rose
        assert math.isnan(pca.pcr_comparison(t_pre, t_post, meta, "one"))  # a constant covariate
        assert math.isnan(pca.pcr_comparison(t_pre, t_post, meta, "one", scale=False))
        assert _close(pca.pcr_comparison(t_post, t_pre, meta, "species", scale=False), after - before)
        # `pre` may have another width than the embeddings
        assert 0.0 < pca.pcr_comparison(torch.from_numpy(np.ascontiguousarray(X[:, :5])), t_post, meta, "species") <= 1.0


def _tool():
    spec = importlib.util.spec_from_file_location("pc_regression_tool", os.path.join(ROOT, "tools", "pc_regression.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_and_csv_writers_on_a_directory_and_an_h5(tmp_path, monkeypatch, capsys):
    from mmvae_amd import backend, pca
    from mmvae_amd import predictions as P

    tool = _tool()
    monkeypatch.delenv("DIRECTORY", raising=False)
    X, batch = R.scaled_batches(n=200, dim=6)
    meta = _frame(X, batch)
    np.savez(tmp_path / "z_embeddings.npz", embeddings=X)
    meta.to_pickle(tmp_path / "z_metadata.pkl")
    a = tool.parse_args(["--directory", str(tmp_path), "--keys", "z", "--covariates", "species", "--covariates", "noise"])
    assert (a.covariates, a.keys, a.save_dir, a.n_comps) == (["species", "noise"], ["z"], None, None)
    assert tool.parse_args(["--directory", str(tmp_path), "--keys", "z"]).covariates == ["species"]
    with pytest.raises(SystemExit):
        tool.parse_args(["--directory", str(tmp_path / "absent"), "--keys", "z"])
    out_dir = tmp_path / "tables"
    with backend.cpu_plumbing():
        assert tool.main(["--directory", str(tmp_path), "--keys", "z", "--covariates", "species", "--covariates",
                          "total_counts", "--n_comps", "4", "--save_dir", str(out_dir)]) == 0
        want = pca.pc_regression(torch.from_numpy(X), meta, ("species", "total_counts"), 4)
    printed = capsys.readouterr().out.split()
    names = ["pcr.z.csv", "pcr.z.components.csv"]
    assert printed == [str(out_dir / n) for n in names] and all(os.path.exists(p) for p in printed)
    table = pd.read_csv(out_dir / names[0])
    assert tuple(table.columns) == pca.SUMMARY_COLUMNS and table["covariate"].tolist() == ["species", "total_counts"]
    assert table["kind"].tolist() == ["categorical", "numeric"] and table["n_comps"].tolist() == [4, 4]
    assert _close(table["pcr"], want.summary["pcr"], 1e-12)
    comps = pd.read_csv(out_dir / names[1])
    assert list(comps.columns) == ["pc", "explained_variance_ratio", "r2.species", "r2.total_counts"] and len(comps) == 4
    assert _close(comps["r2.species"], want.per_component["r2.species"], 1e-12)
    # the predictions.h5 form: the same numbers next to the file
    h5 = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(X, meta[["species", "noise"]], h5, "z")
    with backend.cpu_plumbing():
        assert tool.main(["--directory", h5, "--keys", "z", "--n_comps", "4"]) == 0
    assert capsys.readouterr().out.split() == [str(tmp_path / n) for n in names]
    assert _close(pd.read_csv(tmp_path / names[0])["pcr"][0], table["pcr"][0], 1e-12)


def test_trainer_pc_regression_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend, pca
    from mmvae_amd.trainer import Trainer
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    with backend.cpu_plumbing():
        model = MU.build_mirror(case, "cpu", str(tmp_path), use_engine=True)
        T = len(case["schedule"]) - 1
        MU.load_state(model, z, f"step{T}/sd/")
        x, _, _, _ = H.step_inputs(z, T)
        eid = str(z["eval/expert_id"])
        B = x.shape[0]
        batches = [(x, pd.DataFrame({"group": ["a"] * B, "depth": np.arange(B, dtype=np.float64)}), eid),
                   (x.flip(0) * 0.5, pd.DataFrame({"group": ["b"] * B, "depth": np.arange(B, dtype=np.float64) + 0.5}), eid)]
        out = Trainer().pc_regression(model, batches, covariates=("group", "depth", "species"), n_comps=2)
    assert isinstance(out, pca.PCRResult) and out.fit.n_rows == 2 * B and out.fit.components.shape[0] == 2
    assert out.summary["covariate"].tolist() == ["group", "depth", "species"]
    assert out.summary["kind"].tolist() == ["categorical", "numeric", "categorical"]
    assert out.summary["n_classes"].tolist() == [2, 0, 1] and out.summary["n_cells"].tolist() == [2 * B] * 3
    assert 0.0 <= out.pcr("group") <= 1.0 + 1e-12 and 0.0 <= out.pcr("depth") <= 1.0 + 1e-12 and math.isnan(out.pcr("species"))
    assert len(out.per_component) == 2
