"""Writes tests/golden/prep_normalize.npz: a small raw-count CSR matrix, what the reference's own normalize_data makes of
it, and the mean / std its get_data_stats reports for the raw matrix
(scripts/data-preprocessing/data_processing_functions.py:12-51).

Runs only where the reference checkout is present:  python tests/golden/make_prep_golden.py /path/to/reference
The reference module is loaded by FILE PATH; the fixture holds numbers only.

The matrix: 37 cells x 211 genes of Poisson counts with a log-normal rate per gene (fp32 values, int32 indices), rows 3
and 36 empty, row 17 holding {16 000 000, 777 215} -- a total of 2^24 - 1, still exact in fp32.  No row with stored
elements sums to zero: the reference's answer there is NaN (mmvae_amd.preprocess writes zeros; tested apart)."""
import importlib.util
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
N_ROWS, N_COLS = 37, 211
EMPTY_ROWS = (3, 36)
BIG_ROW, BIG_VALUES, BIG_COLS = 17, (16000000.0, 777215.0), (5, 190)


def raw_matrix() -> sp.csr_matrix:
    rng = np.random.default_rng(20241020)
    rate = 0.6 * np.exp(rng.standard_normal(N_COLS))
    dense = rng.poisson(rate, size=(N_ROWS, N_COLS)).astype(np.float32)
    for r in EMPTY_ROWS:
        dense[r] = 0.0
    dense[BIG_ROW] = 0.0
    dense[BIG_ROW, list(BIG_COLS)] = BIG_VALUES
    m = sp.csr_matrix(dense)
    m.sort_indices()
    assert m.data.dtype == np.float32 and m.indices.dtype == np.int32
    sums = np.asarray(m.sum(axis=1)).ravel()
    assert all(sums[r] == 0 for r in EMPTY_ROWS) and sums[BIG_ROW] == 2.0 ** 24 - 1
    assert (np.delete(sums, EMPTY_ROWS) > 0).all()
    return m


def main(reference_root: str) -> None:
    path = os.path.join(reference_root, "scripts", "data-preprocessing", "data_processing_functions.py")
    spec = importlib.util.spec_from_file_location("reference_data_processing_functions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    raw = raw_matrix()
    mean, std = mod.get_data_stats(raw)
    done = raw.copy()
    mod.normalize_data(done)
    assert done.data.dtype == np.float32 and np.isfinite(done.data).all()
    assert np.array_equal(done.indptr, raw.indptr) and np.array_equal(done.indices, raw.indices)
    np.savez(os.path.join(HERE, "prep_normalize.npz"), indptr=raw.indptr, indices=raw.indices, data=raw.data,
             shape=np.array(raw.shape, dtype=np.int64), expected=done.data, mean=np.asarray(mean), std=np.asarray(std))
    print(f"{raw.shape[0]} x {raw.shape[1]}, {raw.nnz} stored; mean {mean!r} std {std!r} ({np.asarray(mean).dtype})")


if __name__ == "__main__":
    main(sys.argv[1])
