"""Host-side checks of the count normalisation (no GPU): the C-ABI surface of libmmvae_prep.so and its refusals, the numpy
path of normalize_csr_ against the reference's own output (tests/golden/prep_normalize.npz) bit for bit, RowSumStats
against numpy and the reference's get_data_stats, and SpeciesChunks(normalize="log1p_cpm") on a CPU feed."""
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import prep_cases as PC
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_prep.h")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _prep_lib

    declared = check_surface(_prep_lib.BINDING)
    assert set(declared) == {"mmvae_prep_abi_version", "mmvae_prep_build_arch", "mmvae_prep_csr_log1p_norm_i32",
                             "mmvae_prep_csr_log1p_norm_i64"} == set(_prep_lib.PREP_PROTOTYPES)


def test_versions_constants_and_argument_checks():
    from mmvae_amd import _lib, _prep_lib

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _prep_lib.load_prep()
    assert define("MMVAE_PREP_ABI_VERSION") == 1 == lib.mmvae_prep_abi_version() == _prep_lib.PREP_ABI_VERSION
    assert lib.mmvae_prep_build_arch() == b"gfx950"
    assert define("MMVAE_PREP_ROWS_PER_GROUP") == _prep_lib.PREP_ROWS_PER_GROUP
    assert define("MMVAE_PREP_REG_ELEMS") == _prep_lib.PREP_REG_ELEMS and _prep_lib.PREP_REG_ELEMS % 64 == 0
    # the training library is untouched: same version, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_prep_")]
    inf, nan = float("inf"), float("nan")
    for fn in (lib.mmvae_prep_csr_log1p_norm_i32, lib.mmvae_prep_csr_log1p_norm_i64):
        # (n_rows, nnz, crow, values, target_sum, row_sums, stream): refused before any pointer is used
        for bad in ((0, 10, 16, 16, 1e4, 16), (-1, 10, 16, 16, 1e4, 16), (5, -1, 16, 16, 1e4, 16),
                    (5, 10, None, 16, 1e4, 16), (5, 10, 16, None, 1e4, 16), (5, 10, 16, None, 1e4, None),
                    (5, 10, 16, 16, 0.0, 16), (5, 10, 16, 16, -1.0, 16), (5, 10, 16, 16, inf, 16),
                    (5, 10, 16, 16, -inf, 16), (5, 10, 16, 16, nan, 16), (5, 10, 16, 16, 1e39, 16),
                    (0, 0, None, None, 1e4, None)):
            assert fn(*bad, None) == _prep_lib.ERR_ARG, bad


def _csr(indptr, indices, data, shape, idx=torch.int32):
    return torch.sparse_csr_tensor(torch.from_numpy(np.asarray(indptr)).to(idx), torch.from_numpy(np.asarray(indices)).to(idx),
                                   torch.from_numpy(np.array(data, dtype=np.float32)), size=tuple(int(s) for s in shape))


@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_cpu_path_equals_the_reference_bit_for_bit(idx):
    from mmvae_amd.preprocess import normalize_csr_

    g = PC.golden()
    assert tuple(g["shape"]) == (37, 211) and g["data"].dtype == np.float32 and g["expected"].dtype == np.float32
    lengths = np.diff(g["indptr"])
    assert (lengths == 0).sum() == 2 and np.isfinite(g["expected"]).all()
    big = int(np.flatnonzero(PC.reference_fp64(g["indptr"], g["data"])[1] == 2.0 ** 24 - 1)[0])
    assert sorted(g["data"][g["indptr"][big]:g["indptr"][big + 1]].tolist()) == [777215.0, 16000000.0]
    csr = _csr(g["indptr"], g["indices"], g["data"], g["shape"], idx)
    out, sums = normalize_csr_(csr, return_row_sums=True)
    assert out is csr and sums.dtype == torch.float32 and tuple(sums.shape) == (37,)
    assert np.array_equal(csr.values().numpy().view(np.uint32), g["expected"].view(np.uint32))
    assert np.array_equal(csr.col_indices().numpy(), g["indices"]) and np.array_equal(csr.crow_indices().numpy(), g["indptr"])
    ref, ref_sums = PC.reference_fp64(g["indptr"], g["data"])
    assert np.array_equal(sums.numpy(), ref_sums) and float(sums[big]) == 2.0 ** 24 - 1
    PC.assert_close(csr.values().numpy(), ref, "golden, numpy path")
    assert normalize_csr_(_csr(g["indptr"], g["indices"], g["data"], g["shape"], idx)).layout == torch.sparse_csr


def test_row_sum_stats():
    from mmvae_amd.preprocess import RowSumStats, normalize_csr_

    g = PC.golden()
    _, sums = normalize_csr_(_csr(g["indptr"], g["indices"], g["data"], g["shape"]), return_row_sums=True)
    s64 = sums.numpy().astype(np.float64)
    one = RowSumStats.of(sums)
    assert one.n == 37
    assert abs(one.mean - s64.mean()) <= 1e-12 * s64.mean() and abs(one.std - s64.std()) <= 1e-12 * s64.std()
    # the reference's get_data_stats reduces in fp32: 1e-5 relative is the precision of ITS numbers
    assert g["mean"].dtype == np.float32
    assert abs(one.mean - float(g["mean"])) <= 1e-5 * float(g["mean"])
    assert abs(one.std - float(g["std"])) <= 1e-5 * float(g["std"])
    # fed chunk by chunk: the statistics of all chunks
    rng = np.random.default_rng(3)
    parts = [rng.poisson(900.0, size=n).astype(np.float32) for n in (50, 1, 333)]
    acc = RowSumStats()
    for p in parts:
        acc.update(torch.from_numpy(p))
    acc.update(torch.zeros(0))
    every = np.concatenate(parts).astype(np.float64)
    assert acc.n == 384
    assert abs(acc.mean - every.mean()) <= 1e-12 * every.mean() and abs(acc.std - every.std()) <= 1e-12 * every.std()
    assert np.isnan(RowSumStats().mean) and np.isnan(RowSumStats().std)


def test_stored_zero_rows_give_zeros_not_nan():
    from mmvae_amd.preprocess import normalize_csr_

    indptr = [0, 2, 5, 5, 7]
    data = [3.0, 1.0, 0.0, 0.0, 0.0, 2.0, 2.0]
    csr = _csr(indptr, [0, 1, 0, 1, 2, 1, 2], data, (4, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (numpy's "invalid value" must not leak either)
        _, sums = normalize_csr_(csr, return_row_sums=True)
    v = csr.values().numpy()
    assert np.array_equal(sums.numpy(), np.array([4.0, 0.0, 0.0, 4.0], dtype=np.float32))
    assert np.array_equal(v[2:5], np.zeros(3, dtype=np.float32)) and not np.isnan(v).any()
    ref, _ = PC.reference_fp64(indptr, data)
    PC.assert_close(v, ref, "neighbours of a stored-zero row")
    assert v[0] == np.log1p(np.float32(3.0) * np.float32(1e4) / np.float32(4.0))


def test_normalize_csr_refuses_what_it_cannot_take():
    from mmvae_amd.preprocess import normalize_csr_

    good = _csr([0, 1], [0], [1.0], (1, 2))
    with pytest.raises(ValueError):
        normalize_csr_(good.to_dense())
    with pytest.raises(TypeError):
        normalize_csr_(torch.sparse_csr_tensor(torch.tensor([0, 1]), torch.tensor([0]), torch.tensor([1.0], dtype=torch.float64),
                                               size=(1, 2)))
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError):
            normalize_csr_(good, target_sum=bad)
    assert float(normalize_csr_(good, target_sum=1.0).values()[0]) == np.log1p(np.float32(1.0))


# ------------------------------------------------------------------------------------------------------------ feed
@pytest.fixture(scope="module")
def count_chunks(tmp_path_factory):
    """900 x 211 raw counts as three chunk files of 300 rows, and the same matrix normalised first, written likewise."""
    from mmvae_amd import data as D
    from mmvae_amd.preprocess import _normalize_cpu

    m = PC.count_matrix()
    meta = pd.DataFrame({"row": np.arange(m.shape[0])})
    raw_dir, done_dir = str(tmp_path_factory.mktemp("raw")), str(tmp_path_factory.mktemp("done"))
    D.write_chunks(raw_dir, "human", m, meta, chunk_rows=300, compressed=False)
    done = m.copy()
    _normalize_cpu(done.indptr, done.data, 1e4)
    D.write_chunks(done_dir, "human", done, meta, chunk_rows=300, compressed=False)
    return m, raw_dir, done_dir


def _feed(directory, **kw):
    from mmvae_amd import data as D

    return D.SpeciesChunks(directory, "human_train_counts_*.npz", "human_train_metadata_*.pkl", 64, "human", seed=5, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(return_dense=True), dict(index_dtype=torch.int64, allow_partials=True),
                                dict(device="cpu", prefetch=False)], ids=["csr", "dense", "int64_partials", "cpu_device"])
def test_cpu_feed_yields_what_normalising_the_source_first_yields(count_chunks, kw):
    m, raw_dir, done_dir = count_chunks
    kw = dict(kw)
    device = kw.pop("device", None)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # raw counts: no "does not look like raw counts"
        got = list(_feed(raw_dir, normalize="log1p_cpm", device=device, **kw))
    want = list(_feed(done_dir, device=device, **kw))
    assert len(got) == len(want) == (15 if kw.get("allow_partials") else 12)
    ref = PC.normalized_fp64_dense(m)
    for (x, md, name), (x_w, md_w, _) in zip(got, want):
        pd.testing.assert_frame_equal(md, md_w)
        assert x.layout == x_w.layout and x.dtype == torch.float32
        if x.layout == torch.sparse_csr:
            assert torch.equal(x.crow_indices(), x_w.crow_indices()) and torch.equal(x.col_indices(), x_w.col_indices())
            assert np.array_equal(x.values().numpy().view(np.uint32), x_w.values().numpy().view(np.uint32))
            x = x.to_dense()
        else:
            assert np.array_equal(x.numpy().view(np.uint32), x_w.numpy().view(np.uint32))
        PC.assert_close(x.numpy(), ref[md["row"].to_numpy()], "batch against the fp64 normalisation of its rows")


def test_a_bad_normalize_value_raises(count_chunks):
    _, raw_dir, _ = count_chunks
    for bad in ("log1p", "cpm", True, 1):
        with pytest.raises(ValueError, match="normalize"):
            _feed(raw_dir, normalize=bad)
    with pytest.raises(ValueError, match="target_sum"):
        _feed(raw_dir, normalize="log1p_cpm", target_sum=0.0)
    assert _feed(raw_dir).normalize is None and _feed(raw_dir, normalize=None).target_sum == 1e4


@pytest.mark.parametrize("prefetch", [True, False])
def test_the_not_raw_counts_warning_fires_once(count_chunks, prefetch):
    _, raw_dir, done_dir = count_chunks
    feed = _feed(done_dir, normalize="log1p_cpm", prefetch=prefetch)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):  # two epochs, three chunks each
            assert len(list(feed)) == 12
    hits = [w for w in caught if "does not look like raw counts" in str(w.message)]
    assert len(hits) == 1 and issubclass(hits[0].category, RuntimeWarning)
    assert "human_train_counts_" in str(hits[0].message)
    for directory, kw in ((raw_dir, dict(normalize="log1p_cpm")), (done_dir, dict())):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            list(_feed(directory, prefetch=prefetch, **kw))
        assert not [w for w in caught if "does not look like raw counts" in str(w.message)]


def test_offline_tool_on_the_cpu(count_chunks, tmp_path):
    """tools/normalize_chunks.py --device cpu: normalised npz files of the same names, metadata copied, the per-file table."""
    import importlib.util

    from mmvae_amd import data as D

    m, raw_dir, done_dir = count_chunks
    spec = importlib.util.spec_from_file_location("normalize_chunks", os.path.join(ROOT, "tools", "normalize_chunks.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / "out")
    assert tool.main(["--directory", raw_dir, "--species", "human", "--out", out, "--device", "cpu"]) == 0
    assert tool.main(["--directory", raw_dir, "--species", "human", "--out", raw_dir, "--device", "cpu"]) == 1
    table = pd.read_csv(os.path.join(out, "human_data_distribution.csv"))
    assert list(table.columns) == ["file", "mean", "std"]
    assert list(table["file"]) == [f"human_train_counts_{k}.npz" for k in (1, 2, 3)]
    sums = np.asarray(m.sum(axis=1)).ravel().astype(np.float64)
    for k in range(3):
        got, _ = D.load_chunk(os.path.join(out, f"human_train_counts_{k + 1}.npz"),
                              os.path.join(out, f"human_train_metadata_{k + 1}.pkl"))
        want, _ = D.load_chunk(os.path.join(done_dir, f"human_train_counts_{k + 1}.npz"),
                               os.path.join(done_dir, f"human_train_metadata_{k + 1}.pkl"))
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(np.asarray(got.data).view(np.uint32), np.asarray(want.data).view(np.uint32))
        part = sums[300 * k:300 * (k + 1)]
        assert abs(table["mean"][k] - part.mean()) <= 1e-12 * part.mean()
        assert abs(table["std"][k] - part.std()) <= 1e-12 * part.std()
        with open(os.path.join(out, f"human_train_metadata_{k + 1}.pkl"), "rb") as f, \
                open(os.path.join(raw_dir, f"human_train_metadata_{k + 1}.pkl"), "rb") as g:
            assert f.read() == g.read()
