"""The feed's device-resident chunks on the GPU: the row-gather kernels (`mmvae_csr_gather_rows_*`,
`mmvae_csr_gather_rows_dense_*`) against scipy's row slicing, and `SpeciesChunks(device_chunks=True)` against the host
path batch for batch.  Every result is a pure copy: every comparison is bitwise."""
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

ROW_LISTS = {
    "sixteen_one_repeat": [69, 0, 5, 33, 5, 12, 1, 68, 34, 32, 7, 50, 21, 44, 3, 60],
    "single": [12],
    "all_reversed": list(range(69, -1, -1)),
}
TORCH_IDX = {"int32": torch.int32, "int64": torch.int64}


@pytest.fixture(scope="module")
def matrix():
    """70 x 37, about 20 % dense, fp32; rows 0, 33 and 69 empty, row 5 full."""
    rng = np.random.default_rng(2024)
    dense = (rng.random((70, 37), dtype=np.float32) + 0.25) * (rng.random((70, 37)) < 0.2)
    dense[[0, 33, 69]] = 0.0
    dense[5] = np.arange(1, 38, dtype=np.float32)
    m = sp.csr_matrix(dense.astype(np.float32))
    assert m[5].nnz == 37 and m[0].nnz == m[33].nnz == m[69].nnz == 0 and m.data.dtype == np.float32
    return m


def _device_chunk(m, idx):
    return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)).to(idx).cuda(),
                                   torch.from_numpy(m.indices.astype(np.int64)).to(idx).cuda(),
                                   torch.from_numpy(m.data).cuda(), size=m.shape)


@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("which", list(ROW_LISTS))
def test_gather_rows_equals_scipy_row_slice(matrix, which, idx):
    from mmvae_amd import ops

    rows = ROW_LISTS[which]
    want = matrix[rows]
    chunk = _device_chunk(matrix, TORCH_IDX[idx])
    out_crow = torch.from_numpy(want.indptr.astype(np.int64)).to(TORCH_IDX[idx]).cuda()
    got = ops.csr_gather_rows(chunk, torch.tensor(rows, dtype=torch.int64, device="cuda"), out_crow, want.nnz)
    assert got.layout == torch.sparse_csr and tuple(got.shape) == (len(rows), 37)
    assert got.crow_indices().dtype == got.col_indices().dtype == TORCH_IDX[idx] and got.values().dtype == torch.float32
    assert np.array_equal(got.crow_indices().cpu().numpy(), want.indptr)
    assert np.array_equal(got.col_indices().cpu().numpy(), want.indices)
    assert np.array_equal(got.values().cpu().numpy(), want.data)


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_gather_rows_out_of_range_row_numbers_give_empty_rows(matrix, idx):
    """Row numbers 70 and -1 (outside the chunk) get zero-length segments in out_crow: the kernel must read nothing for
    them and leave their neighbours right."""
    from mmvae_amd import ops

    rows = [4, 70, 5, -1, 6, 70]
    valid = [4, 5, 6]
    want = matrix[valid]
    lengths = [matrix[r].nnz if 0 <= r < 70 else 0 for r in rows]
    crow = np.concatenate([[0], np.cumsum(lengths)])
    chunk = _device_chunk(matrix, TORCH_IDX[idx])
    got = ops.csr_gather_rows(chunk, torch.tensor(rows, dtype=torch.int64, device="cuda"),
                              torch.from_numpy(crow).to(TORCH_IDX[idx]).cuda(), int(crow[-1]))
    assert np.array_equal(got.crow_indices().cpu().numpy(), crow)
    assert np.array_equal(got.col_indices().cpu().numpy(), want.indices)
    assert np.array_equal(got.values().cpu().numpy(), want.data)
    # the dense variant: zero rows there
    dense = ops.csr_gather_rows_dense(chunk, torch.tensor(rows, dtype=torch.int64, device="cuda")).cpu().numpy()
    ref = np.zeros((len(rows), 37), dtype=np.float32)
    ref[[0, 2, 4]] = want.toarray()
    assert np.array_equal(dense, ref)


@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("which", list(ROW_LISTS))
def test_gather_rows_dense_equals_scipy(matrix, which, idx):
    from mmvae_amd import ops

    rows = ROW_LISTS[which]
    want = matrix[rows].toarray()
    chunk = _device_chunk(matrix, TORCH_IDX[idx])
    base = torch.full((len(rows), 39), float("nan"), device="cuda")  # ldo = 39: not a multiple of 4
    out = ops.csr_gather_rows_dense(chunk, torch.tensor(rows, dtype=torch.int64, device="cuda"), out=base[:, :37])
    assert out.data_ptr() == base.data_ptr()
    host = base.cpu().numpy()
    assert np.array_equal(host[:, :37], want), "a missed zero fill would have left NaN"
    assert np.isnan(host[:, 37:]).all(), "nothing may be written behind a row's G columns"
    fresh = ops.csr_gather_rows_dense(chunk, torch.tensor(rows, dtype=torch.int64, device="cuda"))
    assert fresh.is_contiguous() and np.array_equal(fresh.cpu().numpy(), want)


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_gather_rows_dense_crosses_the_column_chunk_boundary(idx):
    """3 x 8200: two 8192-column workgroups per row; stored elements on both sides of the boundary."""
    from mmvae_amd import ops

    dense = np.zeros((3, 8200), dtype=np.float32)
    dense[0, [0, 8191, 8192, 8199]] = [1.0, 2.0, 3.0, 4.0]
    dense[2, [8191, 8192]] = [5.0, 6.0]
    m = sp.csr_matrix(dense)
    chunk = _device_chunk(m, TORCH_IDX[idx])
    rows = [2, 0, 1, 0]
    out = torch.full((4, 8200), float("nan"), device="cuda")
    ops.csr_gather_rows_dense(chunk, torch.tensor(rows, dtype=torch.int64, device="cuda"), out=out)
    assert np.array_equal(out.cpu().numpy(), dense[rows])


# ------------------------------------------------------------------------------------------------ feed equivalence
@pytest.fixture(scope="module")
def chunk_dirs(tmp_path_factory):
    """105 rows x 37 genes with metadata as chunk files of 40, 40 and 25 rows: stored (memory-mapped) and compressed."""
    from mmvae_amd import data as D

    rng = np.random.default_rng(11)
    dense = (rng.random((105, 37), dtype=np.float32) + 0.25) * (rng.random((105, 37)) < 0.2)
    dense[[3, 57]] = 0.0
    meta = pd.DataFrame({"row": np.arange(105), "assay": [f"a{i % 3}" for i in range(105)]})
    dirs = {}
    for compressed in (False, True):
        d = tmp_path_factory.mktemp("compressed" if compressed else "stored")
        D.write_chunks(str(d), "human", sp.csr_matrix(dense.astype(np.float32)), meta, chunk_rows=40,
                       compressed=compressed)
        dirs[compressed] = str(d)
    return dirs


def _feed(directory, device_chunks, **kw):
    from mmvae_amd import data as D

    kw.setdefault("shuffle", True)
    return D.SpeciesChunks(directory, "human_train_counts_*.npz", "human_train_metadata_*.pkl", 16, "human", seed=5,
                           device="cuda", device_chunks=device_chunks, **kw)


def _assert_same_batches(a, b, epochs=2):
    n_total = 0
    for _ in range(epochs):
        got, want = list(a), list(b)
        torch.cuda.synchronize()
        assert len(got) == len(want) and len(want) > 0
        for (x, md, name), (x_w, md_w, name_w) in zip(got, want):
            assert name == name_w == "human"
            pd.testing.assert_frame_equal(md, md_w)
            assert x.is_cuda and x.layout == x_w.layout and tuple(x.shape) == tuple(x_w.shape) and x.dtype == x_w.dtype
            if x.layout == torch.sparse_csr:
                for part, part_w in ((x.crow_indices(), x_w.crow_indices()), (x.col_indices(), x_w.col_indices()),
                                     (x.values(), x_w.values())):
                    assert part.dtype == part_w.dtype and torch.equal(part, part_w)
            else:
                assert torch.equal(x, x_w)
        n_total += len(got)
    return n_total


FEED_CASES = {
    "plain": dict(),
    "allow_partials": dict(allow_partials=True),
    "return_dense": dict(return_dense=True),
    "int64": dict(index_dtype=torch.int64),
    "rank_1_of_2": dict(rank=1, world=2),
    "unshuffled_partials_dense": dict(shuffle=False, allow_partials=True, return_dense=True),
}


@pytest.mark.parametrize("case", list(FEED_CASES))
def test_device_chunks_yield_the_host_path_batches(chunk_dirs, case):
    kw = FEED_CASES[case]
    n = _assert_same_batches(_feed(chunk_dirs[False], True, **kw), _feed(chunk_dirs[False], False, **kw))
    per_epoch = {"plain": 5, "allow_partials": 8, "rank_1_of_2": 2}.get(case)  # 40 -> 2 (+1), 40 -> 2 (+1), 25 -> 1 (+1)
    assert per_epoch is None or n == 2 * per_epoch


def test_device_chunks_from_compressed_files(chunk_dirs):
    """Compressed npz members cannot be memory-mapped: the chunk comes through scipy.sparse.load_npz."""
    _assert_same_batches(_feed(chunk_dirs[True], True), _feed(chunk_dirs[True], False))
    _assert_same_batches(_feed(chunk_dirs[True], True), _feed(chunk_dirs[False], True), epochs=1)


def test_device_chunks_behind_a_prefetcher(chunk_dirs):
    """The producer thread gathers on its own stream; the consumer's stream waits for each batch's event and the
    batch's arrays -- its row pointers are a view of the chunk's table -- are recorded on it."""
    from mmvae_amd import data as D

    a = D.Prefetcher(_feed(chunk_dirs[False], True, allow_partials=True), depth=3, device="cuda")
    b = D.Prefetcher(_feed(chunk_dirs[False], False, allow_partials=True), depth=3, device="cuda")
    assert _assert_same_batches(a, b) == 16


def test_device_chunks_without_the_chunk_thread(chunk_dirs):
    _assert_same_batches(_feed(chunk_dirs[False], True, prefetch=False), _feed(chunk_dirs[False], False, prefetch=False))


def test_chunks_over_the_budget_take_the_host_path(chunk_dirs, monkeypatch):
    from mmvae_amd import ops

    def no_launch(*a, **k):
        raise AssertionError("a chunk over the budget must not be gathered on the device")

    monkeypatch.setattr(ops, "csr_gather_rows", no_launch)
    monkeypatch.setattr(ops, "csr_gather_rows_dense", no_launch)
    feed = _feed(chunk_dirs[False], True, device_chunk_bytes=1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _assert_same_batches(feed, _feed(chunk_dirs[False], False))
    budget = [w for w in caught if "device_chunk_bytes" in str(w.message)]
    assert len(budget) == 1, "one warning per SpeciesChunks object, not per chunk or epoch"
    text = str(budget[0].message)
    assert "human_train_counts_" in text and "= 1:" in text


def test_a_malformed_chunk_is_refused_before_anything_is_launched(tmp_path, monkeypatch):
    from mmvae_amd import data as D, ops

    dense = np.eye(8, 5, dtype=np.float32)
    m = sp.csr_matrix(dense)
    m.indices[2] = 5  # column index == n_cols
    meta = pd.DataFrame({"row": np.arange(8)})
    D.write_chunks(str(tmp_path), "human", sp.csr_matrix((8, 5), dtype=np.float32), meta, chunk_rows=8, compressed=False)
    npz = str(tmp_path / "human_train_counts_1.npz")
    np.savez(npz, indices=m.indices, indptr=m.indptr, format=np.array(b"csr"), shape=np.array([8, 5]), data=m.data)
    monkeypatch.setattr(ops, "csr_gather_rows", lambda *a, **k: pytest.fail("launched"))
    feed = D.SpeciesChunks(str(tmp_path), "human_train_counts_*.npz", "human_train_metadata_*.pkl", 4, "human",
                           device="cuda", device_chunks=True)
    with pytest.raises(ValueError, match=r"human_train_counts_1\.npz.*column index"):
        list(feed)


# ------------------------------------------------------------------------------------------------------- training
def _train_six_steps(root, device_chunks):
    from mmvae_amd import data as D, rng, synthetic
    from mmvae_amd.trainer import Lookahead, MultiModalBatches

    genes = {"human": 203, "mouse": 96}
    model = synthetic.build_model(genes, latent_dim=16, h1=64, h2=32, hv=24, dropout=0.1, seed=0).cuda()
    model.train()
    model.trainer.set_stage("training")
    model.optimizers()
    rng.state(torch.device("cuda", 0))
    rng.reseed(1234)  # the same Philox stream for both feeds
    feeds = {name: D.SpeciesChunks(str(root / name), f"{name}_train_counts_*.npz", f"{name}_train_metadata_*.pkl", 32,
                                   name, seed=3, device="cuda", device_chunks=device_chunks) for name in genes}
    batches = D.Prefetcher(MultiModalBatches(feeds, seed=1, round_robin=True), depth=3, device="cuda")
    losses = []
    for i, batch in enumerate(Lookahead(batches, model)):
        model.training_step(batch, i)
        losses.append((batch[2], model.logged[f"loss/training/{batch[2]}"].detach().clone()))
    model._flush_engine()
    torch.cuda.synchronize()
    assert model._engine, "the captured engine must have run the steps"
    state = {k: v.detach().cpu().clone() for k, v in model.module.state_dict().items()}
    model._engine.close()
    return [(eid, v.cpu()) for eid, v in losses], state


def test_training_from_device_chunks_is_bit_identical(tmp_path):
    from mmvae_amd import data as D, synthetic

    for i, (name, g) in enumerate({"human": 203, "mouse": 96}.items()):
        x = synthetic.synthetic_counts(96, g, seed=11 + i, device="cpu").numpy()
        meta = pd.DataFrame({"cell": [f"{name}_{j}" for j in range(96)], "assay": [f"assay_{j % 3}" for j in range(96)]})
        D.write_chunks(str(tmp_path / name), name, sp.csr_matrix(x), meta, chunk_rows=64, compressed=False)
    losses_h, state_h = _train_six_steps(tmp_path, False)
    losses_d, state_d = _train_six_steps(tmp_path, True)
    assert len(losses_h) == len(losses_d) == 6  # (64 -> 2 batches, 32 -> 1) x 2 modalities
    for (eid_h, v_h), (eid_d, v_d) in zip(losses_h, losses_d):
        assert eid_h == eid_d and torch.isfinite(v_h).all() and torch.equal(v_h, v_d), (eid_h, v_h, v_d)
    assert state_h.keys() == state_d.keys()
    diff = [k for k in state_h if not torch.equal(state_h[k], state_d[k])]
    assert not diff, f"parameters differ after six steps: {diff}"
