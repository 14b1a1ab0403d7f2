"""GPU checks of libmmvae_mix.so (include/mmvae_mix.h) against the independent fp64 restatement
(tests/mix_restatement.py).  Both sides read the same (idx, dist), taken from the restatement's own brute-force kNN and
rounded to fp32: the kNN kernel is not under test here.

Bounds.  On firm rows (the restatement's word: no decision of the calibration lies within 1e-9 of its threshold) beta and
tries are bit-equal -- once the decisions agree the beta sequence is exact arithmetic -- and lisi, conf and cross are
within 2^-22 relative: the fp32 store rounds by 2^-24 and everything in front of it is fp64.  pred is equal wherever the
restatement's winning mass leads by more than 1e-9.  At most 1 % of the rows may be left out as not firm.

Shapes: (N, k) = (5, 4) the fewest neighbours, (70, 64) every lane live, (300, 31), (1030, 16) rows no multiple of the
four of a workgroup; Gaussian points, four clusters, and runs of exact duplicates longer than k (rows whose distances are
all equal: 50 tries, uniform weights).
"""
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch

from tests import mix_restatement as R

pytestmark = pytest.mark.gpu

REL = 2.0 ** -22
PAD = 8  # sentinel elements in front of and behind every output
SHAPES = [(5, 4, 1.5), (70, 64, 21.0), (300, 31, 10.0), (1030, 16, 5.0)]
KINDS = ["gaussian", "clusters", "duplicates"]
BIG = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def reference(kind, N, k, perplexity):
    """Inputs and the restatement's results of one case; computed once and never written to."""
    seed = 100 * k + len(kind)
    dim = 8
    if kind == "gaussian":
        X, cluster = R.gaussian(seed, N, dim), None
    elif kind == "clusters":
        X, cluster = R.clusters(seed, N, dim)
    else:
        X, cluster = R.duplicates(seed, N, dim, group=k + 3), None
    rng = np.random.default_rng(seed + 1)
    idx, dist = R.cosine_knn(X, k)
    label = (cluster if cluster is not None else rng.integers(0, 3, N)).astype(np.int32)
    label[rng.random(N) < 0.1] = -1
    label[idx[N // 2, 1:]] = -1            # a row whose neighbours are all unlabelled
    label[label == 2] = BIG                # codes up to 2^31 - 1
    batch = rng.integers(0, 2, N).astype(np.int32)
    batch[rng.random(N) < 0.05] = -1
    equal = np.full(N, 7, dtype=np.int32)
    distinct = (BIG - np.arange(N)).astype(np.int32)
    beta, tries, firm = R.calibrate(dist, perplexity)
    sum_p2 = np.array([(R.weights(beta[i], R.shifted(dist[i]))[0] ** 2).sum() for i in range(N)])
    pred, conf, cross, margin = R.transfer(idx, dist, beta, batch, label)
    out = dict(idx=idx, dist=dist, label=label, batch=batch, codes=np.stack([label, equal, distinct]), beta=beta,
               tries=tries, firm=firm, lisi_label=R.lisi(idx, dist, beta, label), lisi_distinct=1.0 / sum_p2, pred=pred,
               conf=conf, cross=cross, margin=margin)
    for v in out.values():
        v.setflags(write=False)
    return out


def _lib():
    from mmvae_amd import _mix_lib

    return _mix_lib, _mix_lib.load_mix()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Padded:
    """An output buffer with PAD sentinel elements on both sides of its `n` elements."""

    def __init__(self, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.whole = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device="cuda")
        self.body = self.whole[PAD:PAD + n]

    def ptr(self):
        return self.body.data_ptr()

    def untouched_outside(self):
        return bool((self.whole[:PAD] == self.sentinel).all() and (self.whole[PAD + self.n:] == self.sentinel).all())

    def untouched(self):
        return bool((self.whole == self.sentinel).all())


def run_device(idx, dist, perplexity, codes, batch, label, extra_ld=5):
    """Calibrate, LISI of `codes` [n_cols, N] (both leading dimensions N + extra_ld) and transfer through the C entries,
    into sentinel-padded outputs.  Returns numpy results and checks the sentinels."""
    L, lib = _lib()
    N, k = idx.shape
    n_cols, ld = codes.shape[0], N + extra_ld
    d = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the references are read-only)
    idx_d, dist_d, batch_d, label_d = d(idx), d(dist), d(batch), d(label)
    codes_d = torch.full((n_cols, ld), -5, dtype=torch.int32, device="cuda")
    codes_d[:, :N] = d(codes)
    beta, tries = Padded(N, torch.float64, -7.0), Padded(N, torch.int32, -77)
    lisi = Padded(n_cols * ld, torch.float32, -3.0)
    pred, conf, cross = Padded(N, torch.int32, -99), Padded(N, torch.float32, -5.0), Padded(N, torch.float32, -5.0)
    s = _stream()
    L.check(lib.mmvae_mix_calibrate_f32(N, k, idx_d.data_ptr(), dist_d.data_ptr(), perplexity, beta.ptr(), tries.ptr(), s),
            "calibrate")
    L.check(lib.mmvae_mix_lisi_f32(N, k, idx_d.data_ptr(), dist_d.data_ptr(), beta.ptr(), n_cols, codes_d.data_ptr(), ld,
                                   lisi.ptr(), ld, s), "lisi")
    L.check(lib.mmvae_mix_transfer_f32(N, k, idx_d.data_ptr(), dist_d.data_ptr(), beta.ptr(), batch_d.data_ptr(),
                                       label_d.data_ptr(), pred.ptr(), conf.ptr(), cross.ptr(), s), "transfer")
    torch.cuda.synchronize()
    for name, buf in (("beta", beta), ("tries", tries), ("lisi", lisi), ("pred", pred), ("conf", conf), ("cross", cross)):
        assert buf.untouched_outside(), f"{name}: written outside its rows"
    table = lisi.body.view(n_cols, ld)
    assert bool((table[:, N:] == -3.0).all()), "lisi: written between its rows"
    return dict(beta=beta.body.cpu().numpy(), tries=tries.body.cpu().numpy(), lisi=table[:, :N].cpu().numpy(),
                pred=pred.body.cpu().numpy(), conf=conf.body.cpu().numpy(), cross=cross.body.cpu().numpy())


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= REL * np.abs(want))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N, k, perplexity", SHAPES)
def test_kernels_match_the_restatement(N, k, perplexity, kind):
    ref = reference(kind, N, k, perplexity)
    firm = ref["firm"]
    assert firm.mean() >= 0.99, f"{(~firm).sum()} of {N} rows are not firm"
    got = run_device(ref["idx"], ref["dist"], perplexity, ref["codes"], ref["batch"], ref["label"])
    print(f"{kind} N={N} k={k}: firm {firm.mean():.4f}, tries max {ref['tries'].max()} (device {got['tries'].max()}), "
          f"beta equal {np.mean(got['beta'] == ref['beta']):.4f}, "
          f"lisi rel err max {np.nanmax(np.abs(got['lisi'][0] - ref['lisi_label']) / ref['lisi_label']):.3e}")
    assert np.array_equal(got["beta"][firm], ref["beta"][firm])
    assert np.array_equal(got["tries"][firm], ref["tries"][firm])
    # three columns in one launch: labels with gaps (and one row without a labelled neighbour), one class, all distinct
    assert close(got["lisi"][0], ref["lisi_label"])[firm].all()
    assert np.isnan(got["lisi"][0][N // 2]) and np.isnan(ref["lisi_label"][N // 2])
    assert (got["lisi"][1] == 1.0).all()
    assert close(got["lisi"][2], ref["lisi_distinct"])[firm].all()
    assert np.isfinite(got["lisi"][1:]).all()
    # transfer
    sure = firm & (ref["margin"] > 1e-9)
    assert np.array_equal(got["pred"][sure], ref["pred"][sure])
    assert np.array_equal((got["pred"] < 0)[firm], (ref["pred"] < 0)[firm])
    assert close(got["conf"], ref["conf"])[firm].all() and close(got["cross"], ref["cross"])[firm].all()
    lonely = ref["pred"] < 0
    assert (got["conf"][lonely] == 0).all() and (got["cross"][lonely] == 0).all()
    # one column alone gives the same bits as the first of three, and a second run the same bits as the first
    alone = run_device(ref["idx"], ref["dist"], perplexity, ref["codes"][:1], ref["batch"], ref["label"], extra_ld=0)
    assert np.array_equal(alone["lisi"][0], got["lisi"][0], equal_nan=True)
    for name in ("beta", "tries", "pred", "conf", "cross"):
        assert np.array_equal(alone[name], got[name], equal_nan=True), name
    if kind == "duplicates":
        whole = np.arange(N) < (N // (k + 3)) * (k + 3) if N >= k + 3 else np.ones(N, dtype=bool)
        assert (got["tries"][whole] == 50).all() and (got["beta"][whole] == 2.0 ** 50).all()


def test_rows_of_equal_distances_have_uniform_weights_and_ties_go_to_the_smaller_code():
    N, k, perplexity = 19, 16, 5.0
    X = R.duplicates(3, N, 6, group=N)
    idx, dist = R.cosine_knn(X, k)
    assert (dist[:, 1:] == dist[:, 1:2]).all()
    batch = np.ones(N, dtype=np.int32)
    batch[18] = 0  # its neighbours are rows 0 .. 14, all of the other batch; no other row has row 18 among its 15
    label = np.array([5] * 7 + [3] * 7 + [9] + [1] * 4, dtype=np.int32)
    distinct = np.arange(N, dtype=np.int32)
    got = run_device(idx, dist, perplexity, np.stack([label, distinct]), batch, label)
    beta, tries, firm = R.calibrate(dist, perplexity)
    assert firm.all() and (tries == 50).all() and (beta == 2.0 ** 50).all()
    assert np.array_equal(got["beta"], beta) and np.array_equal(got["tries"], tries)
    assert close(got["lisi"][1], np.full(N, 15.0)).all()  # uniform weights on 15 distinct codes: 1 / (15 / 225)
    assert close(got["lisi"][0], R.lisi(idx, dist, beta, label)).all()
    rpred, rconf, rcross, margin = R.transfer(idx, dist, beta, batch, label)
    assert margin[18] == 0.0 and rpred[18] == 3   # seven votes of 1/15 each for 5 and for 3, 5 first in rank
    assert got["pred"][18] == 3
    assert close(got["conf"][18], 7.0 / 15.0) and close(got["cross"][18], 1.0)
    assert (got["pred"][:18] == -1).all() and (got["conf"][:18] == 0).all() and (got["cross"][:18] == 0).all()
    assert np.array_equal(got["pred"], rpred) and close(got["cross"], rcross).all()


def test_refusals_leave_the_outputs_untouched():
    L, lib = _lib()
    N, k = 40, 16
    idx = torch.zeros((N, 65), dtype=torch.int32, device="cuda")
    dist = torch.zeros((N, 65), dtype=torch.float32, device="cuda")
    codes = torch.zeros((2, N), dtype=torch.int32, device="cuda")
    beta_in = torch.ones(N, dtype=torch.float64, device="cuda")
    beta, tries = Padded(N, torch.float64, -7.0), Padded(N, torch.int32, -77)
    lisi = Padded(2 * N, torch.float32, -3.0)
    pred, conf, cross = Padded(N, torch.int32, -99), Padded(N, torch.float32, -5.0), Padded(N, torch.float32, -5.0)
    s = _stream()
    i, d, c, b = idx.data_ptr(), dist.data_ptr(), codes.data_ptr(), beta_in.data_ptr()
    cal = lambda *a: lib.mmvae_mix_calibrate_f32(*a, s)  # noqa: E731
    refused = [cal(N, 2, i, d, 1.5, beta.ptr(), tries.ptr()), cal(N, 65, i, d, 21.0, beta.ptr(), tries.ptr()),
               cal(N, k, i, d, 1.0, beta.ptr(), tries.ptr()), cal(N, k, i, d, float(k - 1), beta.ptr(), tries.ptr()),
               cal(N, k, i, d, float("nan"), beta.ptr(), tries.ptr()), cal(0, k, i, d, 5.0, beta.ptr(), tries.ptr()),
               cal(N, k, None, d, 5.0, beta.ptr(), tries.ptr()), cal(N, k, i, None, 5.0, beta.ptr(), tries.ptr()),
               cal(N, k, i, d, 5.0, None, tries.ptr()), cal(N, k, i, d, 5.0, beta.ptr(), None)]
    li = lambda *a: lib.mmvae_mix_lisi_f32(*a, s)  # noqa: E731
    refused += [li(N, 2, i, d, b, 2, c, N, lisi.ptr(), N), li(N, 65, i, d, b, 2, c, N, lisi.ptr(), N),
                li(N, k, i, d, b, 0, c, N, lisi.ptr(), N), li(N, k, i, d, b, 9, c, N, lisi.ptr(), N),
                li(N, k, i, d, b, 2, c, N - 1, lisi.ptr(), N), li(N, k, i, d, b, 2, c, N, lisi.ptr(), N - 1),
                li(N, k, i, d, None, 2, c, N, lisi.ptr(), N), li(N, k, i, d, b, 2, None, N, lisi.ptr(), N),
                li(N, k, i, d, b, 2, c, N, None, N)]
    tr = lambda *a: lib.mmvae_mix_transfer_f32(*a, s)  # noqa: E731
    cp = codes.data_ptr()
    refused += [tr(N, 2, i, d, b, cp, cp, pred.ptr(), conf.ptr(), cross.ptr()),
                tr(N, 65, i, d, b, cp, cp, pred.ptr(), conf.ptr(), cross.ptr()),
                tr(N, k, i, d, b, None, cp, pred.ptr(), conf.ptr(), cross.ptr()),
                tr(N, k, i, d, b, cp, None, pred.ptr(), conf.ptr(), cross.ptr()),
                tr(N, k, i, d, b, cp, cp, None, conf.ptr(), cross.ptr()),
                tr(N, k, i, d, b, cp, cp, pred.ptr(), None, cross.ptr()),
                tr(N, k, i, d, b, cp, cp, pred.ptr(), conf.ptr(), None)]
    torch.cuda.synchronize()
    assert refused == [L.ERR_ARG] * len(refused), refused
    for name, buf in (("beta", beta), ("tries", tries), ("lisi", lisi), ("pred", pred), ("conf", conf), ("cross", cross)):
        assert buf.untouched(), name


def test_python_entries_run_the_library_on_strided_codes():
    from mmvae_amd import mixing

    N, k, perplexity = 300, 31, 10.0
    ref = reference("clusters", N, k, perplexity)
    got = run_device(ref["idx"], ref["dist"], perplexity, ref["codes"], ref["batch"], ref["label"])
    idx, dist = torch.from_numpy(ref["idx"].copy()).cuda(), torch.from_numpy(ref["dist"].copy()).cuda()
    wide = torch.full((3, N + 9), -4, dtype=torch.int32, device="cuda")
    wide[:, :N] = torch.from_numpy(ref["codes"].copy()).cuda()
    codes = wide[:, :N]                      # ldc = N + 9, no copy
    beta, tries = mixing.calibrate(idx, dist, perplexity)
    assert beta.dtype == torch.float64 and np.array_equal(beta.cpu().numpy(), got["beta"])
    assert np.array_equal(tries.cpu().numpy(), got["tries"])
    values = mixing.lisi(idx, dist, codes, beta=beta)
    assert values.dtype == torch.float32 and values.shape == (3, N)
    assert np.array_equal(values.cpu().numpy(), got["lisi"], equal_nan=True)
    one = mixing.lisi(idx, dist, codes[0], perplexity)  # calibrated inside
    assert one.shape == (N,) and np.array_equal(one.cpu().numpy(), got["lisi"][0], equal_nan=True)
    ten = mixing.lisi(idx, dist, codes[0].repeat(10, 1), beta=beta)  # more columns than one launch takes
    assert ten.shape == (10, N) and all(torch.equal(ten[c].nan_to_num(-1.0), one.nan_to_num(-1.0)) for c in range(10))
    batch, label = torch.from_numpy(ref["batch"].copy()).cuda(), codes[0]
    pred, conf, cross = mixing.label_transfer(idx, dist, batch, label, beta=beta)
    assert np.array_equal(pred.cpu().numpy(), got["pred"])
    assert np.array_equal(conf.cpu().numpy(), got["conf"], equal_nan=True)
    assert np.array_equal(cross.cpu().numpy(), got["cross"])
    wild = idx.clone()
    wild[7, 3] = N
    with pytest.raises(ValueError, match="neighbour indices"):
        mixing.lisi(wild, dist, codes, beta=beta)
    with pytest.raises(TypeError, match="float32"):
        mixing.calibrate(idx, dist.double(), perplexity)


def _two_clusters():
    X, cluster = R.clusters(21, 400, 16, n_clusters=2, spread=0.05)
    return X.astype(np.float32), cluster


def test_integration_metrics_when_the_batches_are_the_clusters():
    from mmvae_amd import mixing

    X, cluster = _two_clusters()
    assert min((cluster == 0).sum(), (cluster == 1).sum()) > 64
    meta = pd.DataFrame({"species": np.where(cluster == 0, "human", "mouse"),
                         "cell_type": [f"t{i % 3}" for i in range(400)]})
    out = mixing.integration_metrics(torch.from_numpy(X).cuda(), meta)
    assert out.idx.shape == (400, 64) and out.lisi.is_cuda and out.lisi.shape == (2, 400)
    assert bool((out.lisi[0] == 1.0).all()), "every neighbourhood holds one batch"
    assert out.summary["median_lisi"][0] == 1.0 and out.summary["scaled_lisi"][0] == 0.0
    assert bool((out.cross["cell_type"] == 0).all() and (out.pred["cell_type"] == -1).all())
    assert bool((out.conf["cell_type"] == 0).all())
    assert out.transfer_summary["share_without_neighbour"].tolist() == [1.0, 1.0, 1.0]
    assert out.transfer_summary["n_scored"].tolist() == [0, 0, 0]
    assert int(out.confusion["cell_type"].values.sum()) == 0


def test_integration_metrics_when_the_batches_are_interleaved():
    from mmvae_amd import mixing

    X, cluster = _two_clusters()
    meta = pd.DataFrame({"species": np.where(np.arange(400) % 2 == 0, "human", "mouse"),
                         "cell_type": np.where(cluster == 0, "B", "T")})
    out = mixing.integration_metrics(torch.from_numpy(X).cuda(), meta)
    idx, dist = out.idx.cpu().numpy(), out.dist.cpu().numpy()  # the restatement runs on the kernel's own graph
    batch, label = out.codes[0].cpu().numpy(), out.codes[1].cpu().numpy()
    assert np.array_equal(batch, np.arange(400) % 2) and np.array_equal(label, cluster)
    beta, tries, firm = R.calibrate(dist, 21.0)
    assert firm.mean() >= 0.99
    assert np.array_equal(out.beta.cpu().numpy()[firm], beta[firm])
    assert np.array_equal(out.tries.cpu().numpy()[firm], tries[firm])
    lisi = out.lisi.cpu().numpy()
    assert close(lisi[0], R.lisi(idx, dist, beta, batch))[firm].all()
    assert close(lisi[1], R.lisi(idx, dist, beta, label))[firm].all() and (lisi[1] == 1.0).all()
    pred, conf, cross, margin = R.transfer(idx, dist, beta, batch, label)
    sure = firm & (margin > 1e-9)
    assert np.array_equal(out.pred["cell_type"].cpu().numpy()[sure], pred[sure])
    assert close(out.conf["cell_type"].cpu().numpy(), conf)[sure].all()
    assert close(out.cross["cell_type"].cpu().numpy(), cross)[firm].all()
    assert out.transfer_summary["accuracy"].tolist() == [1.0, 1.0, 1.0]
    assert out.transfer_summary["n_scored"].tolist() == [200, 200, 400]
    assert out.confusion["cell_type"].values.tolist() == [[int((cluster == 0).sum()), 0], [0, int((cluster == 1).sum())]]
    want = pd.Series(lisi[0].astype(np.float64))
    assert math.isclose(out.summary["mean_lisi"][0], want.mean(), rel_tol=1e-12)
    # about 21 effective neighbours of two even batches: 1 / (1/2 + 1/42) = 1.9 expected
    assert out.summary["median_lisi"][0] > 1.5 and out.summary["n_classes"].tolist() == [2, 2]
