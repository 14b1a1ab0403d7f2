"""Inputs and the fp64 statement of the count normalisation, shared by tests/test_prep_host.py and tests/test_prep_gpu.py.
Everything here is numpy: nothing of mmvae_amd is imported."""
import os

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_normalize.npz")

# Against the fp64 evaluation: two fp32 roundings in multiply and divide plus one in the sum when it is inexact
# (<= 3 * 2^-24), log1p's condition number <= 1, log1pf <= 2 ulp (<= 4 * 2^-24): 7 * 2^-24 = 4.2e-7.
REL_TOL = 5e-7


def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def reference_fp64(indptr, data, target_sum=1e4):
    """(normalised values, fp32 row sums): log1p(v * t / sum v) per row, evaluated in fp64 (t = the fp32 value of
    target_sum); zeros for a row whose stored values sum to 0.  The row sums are fl32 of the fp64 sums."""
    indptr = np.asarray(indptr, dtype=np.int64)
    d = np.asarray(data, dtype=np.float64)
    length = np.diff(indptr)
    sums = np.array([d[a:b].sum() for a, b in zip(indptr[:-1], indptr[1:])], dtype=np.float64)
    per = np.repeat(sums, length)
    t = float(np.float32(target_sum))
    lo, hi = int(indptr[0]), int(indptr[-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.log1p(d[lo:hi] * t / per)
    out[per == 0] = 0.0
    return out, sums.astype(np.float32)


def assert_close(got, ref, what=""):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    worst = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if ref.size else 0.0
    assert (err <= REL_TOL * np.abs(ref)).all(), f"{what}: worst relative error {worst:.3e} > {REL_TOL}"


def geometry_case(reg_elems: int, rows_per_group: int):
    """(indptr int64, data fp32, lengths): integer counts in rows of the lengths that matter to a wave-per-row kernel --
    around one and two passes of 64 lanes, around the register-cache boundary `reg_elems`, a loop of many passes, a row
    of 211, a row of stored ZEROS between ordinary neighbours.  First and last row empty; row starts cover every offset
    mod 4; the row count is one more than a multiple of the rows per workgroup."""
    lengths = [0, 1, 2, 63, 64, 65, 127, 128, 129, reg_elems - 1, reg_elems, reg_elems + 1, 5000, 211, 7, 3, 0]
    zero_row = 15
    assert len(lengths) % rows_per_group == 1
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    assert {int(s) % 4 for s, n in zip(indptr[:-1], lengths) if n} == {0, 1, 2, 3}
    rng = np.random.default_rng(77)
    data = (1 + rng.poisson(3.0, size=int(indptr[-1]))).astype(np.float32)
    data[rng.random(data.size) < 0.01] = 4099.0  # a few large counts
    data[indptr[zero_row]:indptr[zero_row + 1]] = 0.0
    return indptr, data, lengths, zero_row


def count_matrix(n_rows=900, n_cols=211, seed=5):
    """Raw Poisson counts with a log-normal rate per gene as scipy CSR (fp32): row 7 empty, row 11 full (211 stored)."""
    rng = np.random.default_rng(seed)
    rate = 0.4 * np.exp(rng.standard_normal(n_cols))
    dense = rng.poisson(rate, size=(n_rows, n_cols)).astype(np.float32)
    dense[7] = 0.0
    dense[11] = 1.0 + rng.poisson(2.0, size=n_cols)
    m = sp.csr_matrix(dense)
    m.sort_indices()
    assert m[11].nnz == n_cols and m[7].nnz == 0
    return m


def normalized_fp64_dense(m):
    """Dense fp64 normalisation of a scipy CSR count matrix (rows without counts stay zero)."""
    out, _ = reference_fp64(m.indptr, m.data)
    return sp.csr_matrix((out, m.indices, m.indptr), shape=m.shape).toarray()


def ratio_sweep_case(n_rows=1 << 18, seed=9):
    """(indptr, data, fp64 reference, fp32 row sums): rows of TWO stored values of log-uniform magnitude (1e-7 .. 1e7, not
    integers), so that the argument of log1p, 1e4 v / (v + w), sweeps 1e-10 .. 1e4 densely -- around 1 + x = 2 and through
    the range where 1 + x rounds x away.  The fp64 sum of two fp32 values is exact: the row sum is its fl32."""
    rng = np.random.default_rng(seed)
    data = (10.0 ** rng.uniform(-7.0, 7.0, size=2 * n_rows)).astype(np.float32)
    data[:64] = np.float32(1.0)  # (x = 5000 exactly)
    d = data.astype(np.float64).reshape(n_rows, 2)
    sums = d.sum(axis=1)
    ref = np.log1p(d * 1e4 / sums[:, None]).reshape(-1)
    return np.arange(0, 2 * n_rows + 1, 2, dtype=np.int64), data, ref, sums.astype(np.float32)
