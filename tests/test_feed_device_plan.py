"""Host side of the feed's device-resident chunks (`SpeciesChunks(device_chunks=True)`): the per-chunk table of the
batches' row pointers, the host validation of a chunk, and the argument / device checks.  No GPU needed."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from mmvae_amd import data as D


def _chunk(n, g, seed):
    rng = np.random.default_rng(seed)
    dense = (rng.random((n, g), dtype=np.float32) + 0.5) * (rng.random((n, g)) < 0.2)
    dense[n // 2] = 0.0  # an empty row
    return sp.csr_matrix(dense.astype(np.float32))


@pytest.mark.parametrize("n,B", [(70, 16), (64, 16), (5, 16), (16, 16), (33, 1)])
@pytest.mark.parametrize("allow_partials", [False, True])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_batch_row_pointers_match_scipy_slices(n, B, allow_partials, dtype):
    m = _chunk(n, 37, seed=n + B)
    order = np.random.default_rng(7).permutation(n).astype(np.int64)
    table, nnz, n_rows = D.batch_row_pointers(m.indptr, order, B, allow_partials, dtype)
    want = [order[i:i + B] for i in range(0, n, B) if i + B <= n or allow_partials]
    assert table.dtype == dtype and table.shape == (len(want), B + 1)
    assert len(nnz) == len(n_rows) == len(want)
    assert all(type(v) is int for v in nnz) and all(type(v) is int for v in n_rows)
    for k, rows in enumerate(want):
        ref = m[rows]  # scipy's own row slice of the permuted chunk
        assert n_rows[k] == len(rows) and nnz[k] == ref.nnz
        assert np.array_equal(table[k, :len(rows) + 1], ref.indptr)
    if n < B:  # a chunk shorter than one batch: one short batch with partials, none without
        assert len(want) == (1 if allow_partials else 0)


def test_batch_row_pointers_identity_order_and_overflow():
    m = _chunk(40, 11, seed=3)
    table, nnz, _ = D.batch_row_pointers(m.indptr, np.arange(40), 8)
    assert table.dtype == np.int32 and sum(nnz) == m.nnz
    for k in range(5):
        assert np.array_equal(table[k], m.indptr[8 * k:8 * k + 9] - m.indptr[8 * k])
    # row lengths whose running sum leaves int32: refused for int32 tables, fine for int64
    indptr = np.array([0, 2 ** 30, 2 ** 31, 2 ** 31 + 5], dtype=np.int64)
    with pytest.raises(ValueError, match="int64"):
        D.batch_row_pointers(indptr, np.arange(3), 3, dtype=np.int32)
    table, nnz, _ = D.batch_row_pointers(indptr, np.arange(3), 3, dtype=np.int64)
    assert nnz == [2 ** 31 + 5] and table[0].tolist() == indptr.tolist()


def test_validate_csr_chunk_names_the_file_on_each_malformed_case():
    m = _chunk(20, 9, seed=1)
    indptr, indices, data = m.indptr.copy(), m.indices.copy(), m.data.copy()
    D.validate_csr_chunk(indptr, indices, data, 9, "ok.npz")  # the valid chunk passes

    bad = indptr.copy()
    bad[0] = 1
    with pytest.raises(ValueError, match=r"first\.npz.*indptr\[0\]"):
        D.validate_csr_chunk(bad, indices, data, 9, "first.npz")

    bad = indptr.copy()
    bad[3] = indptr[-1] + 1  # an interior row pointer past its successor
    with pytest.raises(ValueError, match=r"decr\.npz.*decreases"):
        D.validate_csr_chunk(bad, indices, data, 9, "decr.npz")

    with pytest.raises(ValueError, match=r"len\.npz.*indptr\[-1\]"):
        D.validate_csr_chunk(indptr, indices[:-1], data[:-1], 9, "len.npz")
    with pytest.raises(ValueError, match=r"len\.npz.*indptr\[-1\]"):
        D.validate_csr_chunk(indptr, indices, data[:-1], 9, "len.npz")

    for v in (9, -1):
        bad = indices.copy()
        bad[len(bad) // 2] = v
        with pytest.raises(ValueError, match=r"col\.npz.*column index"):
            D.validate_csr_chunk(indptr, bad, data, 9, "col.npz")


def test_device_chunks_need_a_gpu_device(tmp_path):
    m = _chunk(20, 9, seed=2)
    D.write_chunks(str(tmp_path), "human", m, pd.DataFrame({"row": np.arange(20)}), chunk_rows=20)
    args = (str(tmp_path), "human_train_counts_*.npz", "human_train_metadata_*.pkl", 4, "human")
    with pytest.raises(ValueError, match="device_chunks"):
        D.SpeciesChunks(*args, device_chunks=True)
    with pytest.raises(ValueError, match="device_chunks"):
        D.SpeciesChunks(*args, device="cpu", device_chunks=True)
    feed = D.SpeciesChunks(*args)  # the default stays the host path
    assert feed.device_chunks is False and feed.device_chunk_bytes is None
    assert len(list(feed)) == 5


def test_gather_ops_refuse_cpu_tensors():
    from mmvae_amd import _lib, ops

    m = _chunk(20, 9, seed=4)
    chunk = torch.sparse_csr_tensor(torch.from_numpy(m.indptr), torch.from_numpy(m.indices), torch.from_numpy(m.data),
                                    size=m.shape)
    rows = torch.arange(4, dtype=torch.int64)
    out_crow = torch.from_numpy(m[:4].indptr.copy())
    with pytest.raises(_lib.HipLibraryError, match="CPU"):
        ops.csr_gather_rows(chunk, rows, out_crow, int(out_crow[-1]))
    with pytest.raises(_lib.HipLibraryError, match="CPU"):
        ops.csr_gather_rows_dense(chunk, rows)


def test_gather_entry_points_check_their_arguments():
    """MMVAE_ERR_ARG before anything is launched: null pointers, B <= 0, B > 65535, negative counts, ldo < G."""
    from mmvae_amd import _lib

    lib = _lib.load()
    p = 4096  # never dereferenced: every call below is refused on the host
    for fn in (lib.mmvae_csr_gather_rows_i32, lib.mmvae_csr_gather_rows_i64):
        good = [4, 10, 20, p, p, p, p, p, 8, p, p, None]
        for pos, bad in [(0, 0), (0, -1), (0, 65536), (1, -1), (2, -1), (8, -1), (3, None), (4, None), (5, None),
                         (6, None), (7, None), (9, None), (10, None)]:
            args = list(good)
            args[pos] = bad
            assert fn(*args) == _lib.ERR_ARG, (pos, bad)
    for fn in (lib.mmvae_csr_gather_rows_dense_i32, lib.mmvae_csr_gather_rows_dense_i64):
        good = [4, 37, 10, 20, p, p, p, p, p, 39, None]
        for pos, bad in [(0, 0), (0, 65536), (1, 0), (2, -1), (3, -1), (4, None), (5, None), (6, None), (7, None),
                         (8, None), (9, 36)]:
            args = list(good)
            args[pos] = bad
            assert fn(*args) == _lib.ERR_ARG, (pos, bad)
