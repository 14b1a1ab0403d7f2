"""The count normalisation on the GPU: `mmvae_prep_csr_log1p_norm_*` against an fp64 evaluation of the formula (every
element within PC.REL_TOL = 5e-7 relative; the row sums exactly fl32 of the fp64 sums), and
`SpeciesChunks(normalize="log1p_cpm")` -- device-resident chunks against host-gathered batches, bit for bit."""
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from tests import prep_cases as PC

pytestmark = pytest.mark.gpu

TORCH_IDX = {"int32": torch.int32, "int64": torch.int64}
SENTINEL = -12345.5


def _run(indptr, data, idx, target_sum=1e4, want_sums=True, pad=(5, 7)):
    """The op over `data` placed inside a larger buffer of sentinels (`pad` elements before and after).  Returns (values,
    row sums or None) on the host, after checking that the sentinels and the row pointers are untouched."""
    from mmvae_amd import ops

    n, nnz = len(indptr) - 1, len(data)
    buf = torch.full((pad[0] + nnz + pad[1],), SENTINEL, dtype=torch.float32, device="cuda")
    values = buf[pad[0]:pad[0] + nnz]
    values.copy_(torch.from_numpy(np.asarray(data, dtype=np.float32)))
    crow = torch.from_numpy(np.asarray(indptr, dtype=np.int64)).to(TORCH_IDX[idx]).cuda()
    sums = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device="cuda") if want_sums else None
    out = ops.csr_log1p_normalize_(crow, values, target_sum, sums[1:n + 1] if want_sums else None)
    torch.cuda.synchronize()
    assert out.data_ptr() == values.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:pad[0]] == SENTINEL).all() and (host[pad[0] + nnz:] == SENTINEL).all(), "written outside the values"
    assert np.array_equal(crow.cpu().numpy(), np.asarray(indptr)), "row pointers changed"
    if want_sums:
        s = sums.cpu().numpy()
        assert s[0] == SENTINEL and s[-1] == SENTINEL, "written outside row_sums"
        return host[pad[0]:pad[0] + nnz], s[1:-1]
    return host[pad[0]:pad[0] + nnz], None


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_golden_fixture(idx):
    from mmvae_amd.preprocess import RowSumStats, normalize_csr_

    g = PC.golden()
    ref, ref_sums = PC.reference_fp64(g["indptr"], g["data"])
    got, sums = _run(g["indptr"], g["data"], idx)
    PC.assert_close(got, ref, "golden against fp64")
    assert np.array_equal(sums, ref_sums)
    # the public surface: indices untouched, the row sums' statistics are the reference's get_data_stats
    t = TORCH_IDX[idx]
    csr = torch.sparse_csr_tensor(torch.from_numpy(g["indptr"]).to(t).cuda(), torch.from_numpy(g["indices"]).to(t).cuda(),
                                  torch.from_numpy(g["data"].copy()).cuda(), size=tuple(int(s) for s in g["shape"]))
    out, dev_sums = normalize_csr_(csr, return_row_sums=True)
    assert out is csr and dev_sums.is_cuda
    assert np.array_equal(csr.values().cpu().numpy().view(np.uint32), got.view(np.uint32))
    assert np.array_equal(csr.col_indices().cpu().numpy(), g["indices"])
    assert np.array_equal(csr.crow_indices().cpu().numpy(), g["indptr"])
    st = RowSumStats.of(dev_sums)
    s64 = ref_sums.astype(np.float64)
    assert abs(st.mean - s64.mean()) <= 1e-12 * s64.mean() and abs(st.std - s64.std()) <= 1e-12 * s64.std()
    assert abs(st.mean - float(g["mean"])) <= 1e-5 * float(g["mean"]) and abs(st.std - float(g["std"])) <= 1e-5 * float(g["std"])


@pytest.fixture(scope="module")
def geometry():
    from mmvae_amd._prep_lib import PREP_REG_ELEMS, PREP_ROWS_PER_GROUP

    indptr, data, lengths, zero_row = PC.geometry_case(PREP_REG_ELEMS, PREP_ROWS_PER_GROUP)
    assert {PREP_REG_ELEMS - 1, PREP_REG_ELEMS, PREP_REG_ELEMS + 1, 5000, 211, 0, 1, 2, 63, 64, 65, 127, 128, 129} <= set(lengths)
    assert lengths[0] == 0 and lengths[-1] == 0 and len(lengths) % PREP_ROWS_PER_GROUP == 1
    return indptr, data, zero_row, {t: PC.reference_fp64(indptr, data, t) for t in (1e4, 1.0, 1e6)}


@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("target_sum", [1e4, 1.0, 1e6])
def test_row_lengths_around_every_path(geometry, idx, target_sum):
    indptr, data, zero_row, refs = geometry
    ref, ref_sums = refs[target_sum]
    got, sums = _run(indptr, data, idx, target_sum)
    PC.assert_close(got, ref, f"geometry case, target_sum {target_sum}")
    assert np.array_equal(sums, ref_sums)
    z = slice(int(indptr[zero_row]), int(indptr[zero_row + 1]))
    assert z.stop - z.start == 3 and (got[z] == 0).all() and sums[zero_row] == 0  # stored zeros: zeros, not NaN
    assert (got[:z.start] > 0).all()


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_row_sums_none_and_two_calls_bit_identical(geometry, idx):
    indptr, data, _, refs = geometry
    a, sums = _run(indptr, data, idx)
    b, none = _run(indptr, data, idx, want_sums=False, pad=(2, 3))  # (another alignment of the values)
    assert none is None and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c, sums_c = _run(indptr, data, idx)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(sums.view(np.uint32), sums_c.view(np.uint32))


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_a_single_row_and_row_pointers_that_do_not_start_at_zero(geometry, idx):
    indptr, data, _, _ = geometry
    one = data[:300]
    ref, ref_sums = PC.reference_fp64([0, 300], one)
    got, sums = _run([0, 300], one, idx)
    PC.assert_close(got, ref, "n_rows = 1")
    assert np.array_equal(sums, ref_sums)
    # rows 4 .. 9 of the geometry case through their own slice of the row pointers: nothing outside
    # [crow[0], crow[n_rows]) may change
    sub = indptr[4:11]
    lo, hi = int(sub[0]), int(sub[-1])
    ref, ref_sums = PC.reference_fp64(sub, data)
    got, sums = _run(sub, data, idx)
    assert np.array_equal(got[:lo], data[:lo]) and np.array_equal(got[hi:], data[hi:]), "written outside the rows given"
    PC.assert_close(got[lo:hi], ref, "a slice of the row pointers")
    assert np.array_equal(sums, ref_sums)


def test_cpu_tensors_and_bad_arguments_raise():
    from mmvae_amd import _lib, ops

    crow, val = torch.tensor([0, 2], dtype=torch.int32), torch.ones(2)
    with pytest.raises(_lib.HipLibraryError):
        ops.csr_log1p_normalize_(crow, val)
    with pytest.raises(_lib.HipLibraryError):
        ops.csr_log1p_normalize_(crow.cuda(), val.cuda(), target_sum=0.0)
    with pytest.raises(TypeError):
        ops.csr_log1p_normalize_(crow.cuda().to(torch.int16), val.cuda())
    with pytest.raises(ValueError):
        ops.csr_log1p_normalize_(crow.cuda(), val.cuda(), row_sums=torch.empty(3, device="cuda"))


# ------------------------------------------------------------------------------------------------------------ feed
@pytest.fixture(scope="module")
def count_chunks(tmp_path_factory):
    """900 x 211 raw counts with metadata as three chunk files of 300 rows, and the fp64 normalisation of the matrix."""
    from mmvae_amd import data as D

    m = PC.count_matrix()
    meta = pd.DataFrame({"row": np.arange(m.shape[0])})
    d = str(tmp_path_factory.mktemp("raw"))
    D.write_chunks(d, "human", m, meta, chunk_rows=300, compressed=False)
    return m, d, PC.normalized_fp64_dense(m)


def _feed(directory, device_chunks, **kw):
    from mmvae_amd import data as D

    return D.SpeciesChunks(directory, "human_train_counts_*.npz", "human_train_metadata_*.pkl", 64, "human", seed=5,
                           device="cuda", device_chunks=device_chunks, **kw)


def _parts(x):
    return (x.crow_indices(), x.col_indices(), x.values()) if x.layout == torch.sparse_csr else (x,)


def _assert_identical_and_close(a, b, ref, n_expected):
    got, want = list(a), list(b)
    torch.cuda.synchronize()
    assert len(got) == len(want) == n_expected
    for (x, md, _), (x_w, md_w, _) in zip(got, want):
        pd.testing.assert_frame_equal(md, md_w)
        assert x.is_cuda and x_w.is_cuda and x.layout == x_w.layout
        for p, p_w in zip(_parts(x), _parts(x_w)):
            assert p.dtype == p_w.dtype and torch.equal(p, p_w)  # (values: no NaN, so equal means bit-identical)
        dense = (x.to_dense() if x.layout == torch.sparse_csr else x).cpu().numpy()
        PC.assert_close(dense, ref[md["row"].to_numpy()], "batch against the fp64 normalisation of its raw rows")


@pytest.mark.parametrize("kw", [dict(), dict(return_dense=True), dict(index_dtype=torch.int64),
                                dict(allow_partials=True, return_dense=True)],
                         ids=["csr", "dense", "csr_int64", "dense_partials"])
def test_device_chunks_and_host_gather_yield_identical_normalised_batches(count_chunks, kw):
    _, d, ref = count_chunks
    n = 15 if kw.get("allow_partials") else 12
    _assert_identical_and_close(_feed(d, True, normalize="log1p_cpm", **kw), _feed(d, False, normalize="log1p_cpm", **kw),
                                ref, n)


@pytest.mark.parametrize("dense", [False, True], ids=["csr", "dense"])
def test_a_chunk_over_the_budget_takes_the_host_path_and_yields_the_same_batch(count_chunks, dense, monkeypatch):
    from mmvae_amd import ops

    _, d, ref = count_chunks
    resident = _feed(d, True, normalize="log1p_cpm", return_dense=dense)
    want = list(resident)
    torch.cuda.synchronize()

    def no_launch(*a, **k):
        raise AssertionError("a chunk over the budget must not be gathered on the device")

    monkeypatch.setattr(ops, "csr_gather_rows", no_launch)
    monkeypatch.setattr(ops, "csr_gather_rows_dense", no_launch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (the budget warning)
        _assert_identical_and_close(_feed(d, True, normalize="log1p_cpm", return_dense=dense, device_chunk_bytes=1024),
                                    want, ref, 12)


@pytest.mark.parametrize("device_chunks", [False, True], ids=["host_gather", "device_chunks"])
def test_without_normalize_the_batches_are_the_raw_values(count_chunks, device_chunks):
    """The one assertion about the old path (the feed's default: no `normalize` argument is passed)."""
    m, d, _ = count_chunks
    raw = m.toarray()
    batches = list(_feed(d, device_chunks))
    torch.cuda.synchronize()
    assert len(batches) == 12
    for x, md, _ in batches:
        assert np.array_equal(x.to_dense().cpu().numpy(), raw[md["row"].to_numpy()])


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_the_transform_over_a_dense_sweep_of_ratios(idx):
    """262 144 two-element rows of log-uniform values: the argument of log1p runs from 1e-10 to 1e4.  The kernel's log1p is
    built on the hardware logarithm (csrc/csr_prep.hip: log1p_f32); this is where a weak spot of it would show."""
    indptr, data, ref, ref_sums = PC.ratio_sweep_case()
    got, sums = _run(indptr, data, idx)
    assert np.array_equal(sums, ref_sums)
    rel = np.abs(got.astype(np.float64) - ref) / ref
    print(f"worst relative error over {ref.size} elements: {rel.max():.3e} (bound {PC.REL_TOL})")
    PC.assert_close(got, ref, "ratio sweep")
