"""mmvae_col_pearson_f32 on the GPU: the per-gene Pearson correlation of two [cells, genes] matrices against fp64 numpy
(centred two-pass, NaN where a column is constant).

Bound: |r - expected| <= 5e-7 wherever a correlation exists, NaN positions exact.  The method (five fp64 moments of the
values shifted by the column's first row) measures <= 3e-8 in fp64 emulation on exactly these inputs; the bound is a few
fp32 ulps of a value in [-1, 1] and covers the fp32 store and the device's fp64 sqrt / divide.  fp32 raw moments miss it
by four orders of magnitude (1.4e-2 at mean 100, sigma 1)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 5e-7
# (B, G, mean, sigma): the row counts cross every power-of-two row chunk up to 1 024, the gene counts leave column tail
# groups, the means are the cancellation-prone ones
CASES = [(2, 5, 0.0, 1.0), (33, 61, 0.0, 1.0), (100, 260, 3.0, 1.0), (257, 131, 100.0, 1.0), (1025, 70, 1000.0, 1e-3),
         (2049, 33, 7.3, 1.0)]


def make_inputs(B, G, mean, sigma):
    rng = np.random.default_rng(1)
    a = (mean + sigma * rng.standard_normal((B, G))).astype(np.float32)
    b = (0.5 * a + mean + sigma * rng.standard_normal((B, G))).astype(np.float32)
    a[:, 2] = np.maximum(a[:, 2] - np.float32(mean) - np.float32(2.5 * sigma), np.float32(0.0))  # mostly zeros
    a[:, 0] = 0.0
    b[:, 1] = np.float32(3.1415927)
    return a, b


def expected(a, b):
    """fp64, centred two-pass; NaN where a column of a or of b is constant."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    da, db = a64 - a64.mean(0), b64 - b64.mean(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (da * db).sum(0) / np.sqrt((da * da).sum(0) * (db * db).sum(0))
    r[(a == a[0]).all(0) | (b == b[0]).all(0)] = np.nan
    return r


def check(r, want, what=""):
    got = r.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{what}: max |r - expected| {err:.3g} over {int(ok.sum())} columns, {int((~ok).sum())} NaN")
    assert err <= BOUND, (what, err)
    assert (np.abs(got[ok]) <= 1.0).all()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from mmvae_amd import ops as _ops

    return _ops


@pytest.mark.parametrize("B,G,mean,sigma", CASES)
def test_accuracy_nan_positions_and_self_correlation(ops, B, G, mean, sigma):
    a, b = make_inputs(B, G, mean, sigma)
    want = expected(a, b)
    assert np.isnan(want[0]) and np.isnan(want[1])  # the constant columns
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    r = ops.col_pearson(ta, tb)
    check(r, want, f"({B}, {G}, mean {mean}, sigma {sigma})")
    again = ops.col_pearson(ta, tb)
    assert torch.equal(r.view(torch.int32), again.view(torch.int32))  # bitwise reproducible, NaNs included
    out = torch.full((G,), 7.0, device="cuda")
    assert ops.col_pearson(ta, tb, out=out) is out and torch.equal(out.view(torch.int32), r.view(torch.int32))
    for t, m in ((ta, a), (tb, b)):  # a == b: exactly 1 wherever the column varies
        own = ops.col_pearson(t, t).cpu().numpy()
        varies = ~(m == m[0]).all(0)
        assert np.isnan(own[~varies]).all() and (own[varies] == 1.0).all()


def test_alignment_and_strides(ops):
    B, G, mean, sigma = CASES[2]
    a, b = make_inputs(B, G, mean, sigma)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert ta.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0
    base = ops.col_pearson(ta, tb)
    check(base, expected(a, b), "contiguous, 16-byte regular")
    narrow = ops.col_pearson(ta[:, :259], tb[:, :259])  # 16-byte rows, the last column group straddles the end
    check(narrow, expected(a[:, :259], b[:, :259]), "[:, :259] views")
    assert torch.equal(narrow.view(torch.int32), base[:259].view(torch.int32))
    shifted = []
    for m in (a, b):  # the same values from a base pointer one float off a 16-byte boundary: element-wise loads
        flat = torch.zeros(B * G + 1, device="cuda")
        flat[1:] = torch.from_numpy(m).cuda().flatten()
        shifted.append(flat[1:].view(B, G))
        assert shifted[-1].data_ptr() % 16 == 4
    off = ops.col_pearson(*shifted)
    check(off, expected(a, b), "base pointer offset by one float")
    mixed = ops.col_pearson(ta, shifted[1])
    check(mixed, expected(a, b), "one aligned, one offset operand")
    assert torch.equal(off.view(torch.int32), base.view(torch.int32))


def test_argument_checks_launch_nothing(ops):
    from mmvae_amd import _lib

    lib = _lib.load()
    a = torch.randn(8, 12, device="cuda")
    with pytest.raises(_lib.HipLibraryError, match="MMVAE_ERR_ARG"):
        ops.col_pearson(a[:1], a[:1])
    with pytest.raises(_lib.HipLibraryError):
        ops.col_pearson(a.cpu(), a.cpu())
    with pytest.raises(ValueError):
        ops.col_pearson(a, a[:, :11])
    r = torch.full((12,), 7.0, device="cuda")
    need = lib.mmvae_col_pearson_workspace_bytes(8, 12)
    assert need > 0 and lib.mmvae_col_pearson_workspace_bytes(1, 12) == 0
    ws = torch.zeros(need // 4 + 4, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    calls = {
        "B = 1": (1, 12, p(a), 12, p(a), 12, p(r), p(ws), need, s),
        "lda < G": (8, 12, p(a), 11, p(a), 12, p(r), p(ws), need, s),
        "ldb < G": (8, 12, p(a), 12, p(a), 11, p(r), p(ws), need, s),
        "short workspace": (8, 12, p(a), 12, p(a), 12, p(r), p(ws), need - 8, s),
        "no workspace": (8, 12, p(a), 12, p(a), 12, p(r), None, need, s),
        "null operand": (8, 12, None, 12, p(a), 12, p(r), p(ws), need, s),
    }
    for what, args in calls.items():
        assert lib.mmvae_col_pearson_f32(*args) == _lib.ERR_ARG, what
    torch.cuda.synchronize()
    assert (r == 7.0).all() and (ws == 0).all()  # nothing ran
    assert lib.mmvae_col_pearson_f32(8, 12, p(a), 12, p(a), 12, p(r), p(ws), need, s) == _lib.OK
    torch.cuda.synchronize()
    assert (r == 1.0).all()


def test_reference_shape(ops):
    """(100, 60 530): the reference's SAMPLE_SIZE cells by its human gene count, contiguous -- rows that are no 16-byte
    groups -- with log1p-normalised counts (many all-zero genes) against a noisy copy."""
    from oracle.mmvae_oracle import synthetic_counts

    B, G = 100, 60530
    a = synthetic_counts(B, G).numpy().astype(np.float32)
    b = (a + 0.25 * np.random.default_rng(2).standard_normal((B, G))).astype(np.float32)
    want = expected(a, b)
    assert 0 < int(np.isnan(want).sum()) < G
    r = ops.col_pearson(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    check(r, want, "(100, 60530)")


def test_model_gene_correlation(tmp_path):
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, _ = H.load_case("two_mod_odd")
    model = MU.build_mirror(case, "cuda", str(tmp_path), use_engine=True)
    a, b = make_inputs(100, 260, 3.0, 1.0)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    r, mean_r, n_valid = model.gene_correlation(ta, tb)
    from mmvae_amd import ops

    assert torch.equal(r.view(torch.int32), ops.col_pearson(ta, tb).view(torch.int32))
    assert int(n_valid) == int((~torch.isnan(r)).sum()) == int((~np.isnan(expected(a, b))).sum()) < 260
    assert float(mean_r) == float(torch.nanmean(r)) and not np.isnan(float(mean_r))
    assert np.isnan(float(r.mean()))  # what the reference's plain mean gives as soon as one gene is dead
