"""GPU checks of libmmvae_pca.so (include/mmvae_pca.h) and mmvae_amd.pca against the independent fp64 restatement
(tests/pcr_restatement.py).  Both sides read the same fp32 rows and the same fp32 mean, so both centre to the same numbers
c = fl32(a - mean).

Shapes (N, D, M): (5, 3, 0) below one tile; (70, 8, 1) just past 64 rows; (300, 70, 2) D off 4 and off 64; (1030, 130, 0)
several output tiles and the mirrored triangle; (200, 512, 0) the largest W, reached by D alone; (600, 504, 8) the largest
W with the largest M; (2100, 128, 3) the production D; (4 CHAIN + 37, 16, 0) several chains and row ranges.  The rows are
the Gaussian blobs of `sil_restatement.clusters`, every coordinate shifted by 3 so that centring matters, rounded to
fp32.  Every call has ldx = D + 5 and ldy = M + 3 with NaN in the pad columns, PAD sentinel elements around every output,
and a workspace of exactly the asked size followed by sentinel bytes; a second call with ldx = D gives the same bits.

Bounds (u = 2^-24), from the definitions of the header:
  scatter      |S_uv - S64_uv| <= (CHAIN + 2) u sum_i |c_iu c_iv|: a chain is at most CHAIN fmaf roundings, each relative to
               a partial sum of at most the chain's sum of magnitudes; the fp64 additions of the chains are negligible
               (the + 2).  S == S.T exactly.
  class sums   <= N 2^-52 sum |c| per element: fewer than N fp64 additions on either side, 2^-53 each.
  projection   |score - score64| <= (D + 1) u sum_d |c_id v_pd|: D fmaf roundings.
  variances    sum_i score_ip^2 against lambda_p.  The score of the fp64 component differs from the device's by at most
               b_ip = (D + 2) u sum_d |c_id v_pd| (the chain, and the rounding of the component to fp32), so the sums of
               squares differ by at most sum_i (2 |s_ip| b_ip + b_ip^2); lambda_p = v^T S v for the device's S, which is
               within (CHAIN + 2) u |v|^T T |v| of v^T S64 v (T_uv = sum_i |c_iu c_iv|); eigh is backward stable to
               D 2^-52 lambda_1.
  PCR          at full rank sum_j lambda_j R2_j = tr(B), B the between-class scatter, and sum_j lambda_j = tr(S): no
               eigenvector enters.  tr(S) is a sum of non-negative chains: (CHAIN + 2) u relative; the class sums are fp64.
               2 (CHAIN + 2) u relative is asserted.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from tests import pcr_restatement as P
from tests import sil_restatement as R

pytestmark = pytest.mark.gpu

PAD = 8
U = 2.0 ** -24


def _lib():
    from mmvae_amd import _pca_lib

    return _pca_lib, _pca_lib.load_pca()


def chain():
    from mmvae_amd import _pca_lib

    return _pca_lib.PCA_CHAIN


def shapes():
    return [(5, 3, 0), (70, 8, 1), (300, 70, 2), (1030, 130, 0), (200, 512, 0), (600, 504, 8), (2100, 128, 3),
            (4 * chain() + 37, 16, 0)]


SHAPE_IDS = ["5x3", "70x8+1", "300x70+2", "1030x130", "200x512", "600x504+8", "2100x128+3", "4chains+37x16"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def reference(N, D, M):
    """Inputs and the restatement's moments of one shape; computed once and never written to."""
    seed = 1000 * D + N
    X, cls = R.clusters(seed, N, D, min(8, N))
    X = X.astype(np.float32)
    Y = None
    if M:
        rng = np.random.default_rng(seed + 1)
        Y = (rng.standard_normal((N, M)) * (1.0 + np.arange(M)) + 5.0 + 0.3 * X[:, :1]).astype(np.float32)
    mean = P.mean32(X)
    full = mean if Y is None else np.concatenate([mean, P.mean32(Y)])
    S, T = P.scatter(X, full, Y)
    out = dict(X=X, Y=Y, cls=cls, mean=mean, full=full, S=S, T=T)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


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


def wide_rows(X, extra_ld):
    N, D = X.shape
    wide = torch.full((N, D + extra_ld), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :D] = torch.from_numpy(np.array(X)).cuda()
    return wide


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def workspace(nbytes):
    assert nbytes > 0 and nbytes % 16 == 0
    return torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")


def run_scatter(ref, extra_x=5, extra_y=3):
    L, lib = _lib()
    X, Y = ref["X"], ref["Y"]
    N, D = X.shape
    M = 0 if Y is None else Y.shape[1]
    W = D + M
    wx = wide_rows(X, extra_x)
    wy = wide_rows(Y, extra_y) if M else None
    mean = dev(ref["full"])
    out = Padded(W * W, torch.float64, -5.0)
    nbytes = lib.mmvae_pca_scatter_workspace_bytes(N, D, M)
    assert nbytes <= L.PCA_PARTIAL_CAP
    ws = workspace(nbytes)
    L.check(lib.mmvae_pca_scatter_f32(N, D, wx.data_ptr(), D + extra_x, M, wy.data_ptr() if M else None, M + extra_y if M else 0,
                                      mean.data_ptr(), out.ptr(), ws.data_ptr(), nbytes, _stream()), "mmvae_pca_scatter_f32")
    torch.cuda.synchronize()
    assert out.untouched_outside(), "scatter: written outside its elements"
    assert bool((ws[nbytes:] == 0xAB).all()), "written past the workspace"
    return out.body.cpu().numpy().reshape(W, W)


def run_sums(X, mean, order, run_ptr, extra_x=5):
    L, lib = _lib()
    N, D = X.shape
    C = len(run_ptr) - 1
    wx = wide_rows(X, extra_x)
    mean_d = None if mean is None else dev(mean)
    order_d = Padded(max(len(order), 1), torch.int32, 0)  # (an empty list still needs an address)
    order_d.body[:len(order)] = dev(np.asarray(order, dtype=np.int32))
    run_d = dev(np.asarray(run_ptr, dtype=np.int32))
    out = Padded(C * D, torch.float64, -5.0)
    nbytes = lib.mmvae_pca_group_sums_workspace_bytes(N, D)
    ws = workspace(nbytes)
    L.check(lib.mmvae_pca_group_sums_f64(N, D, wx.data_ptr(), D + extra_x, None if mean is None else mean_d.data_ptr(), C,
                                         order_d.ptr(), run_d.data_ptr(), out.ptr(), ws.data_ptr(), nbytes, _stream()),
            "mmvae_pca_group_sums_f64")
    torch.cuda.synchronize()
    assert out.untouched_outside(), "class sums: written outside their elements"
    assert bool((ws[nbytes:] == 0xAB).all()), "written past the workspace"
    return out.body.cpu().numpy().reshape(C, D)


def run_project(X, mean, comp, extra_x=5, extra_s=3):
    L, lib = _lib()
    N, D = X.shape
    Pn = len(comp)
    wx = wide_rows(X, extra_x)
    scores = torch.full((N + 2, Pn + extra_s), -5.0, dtype=torch.float32, device="cuda")  # (a sentinel row on either side)
    mean_d, comp_d = dev(mean), dev(comp)
    L.check(lib.mmvae_pca_project_f32(N, D, wx.data_ptr(), D + extra_x, mean_d.data_ptr(), Pn, comp_d.data_ptr(),
                                      scores[1].data_ptr(), Pn + extra_s, _stream()), "mmvae_pca_project_f32")
    torch.cuda.synchronize()
    assert bool((scores[0] == -5.0).all() and (scores[-1] == -5.0).all() and (scores[:, Pn:] == -5.0).all()), \
        "scores: written outside their elements"
    return scores[1:-1, :Pn].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("shape", shapes(), ids=SHAPE_IDS)
def test_scatter_meets_its_bound_and_is_symmetric(shape):
    ref = reference(*shape)
    got = run_scatter(ref)
    bound = (chain() + 2) * U * ref["T"]
    err = np.abs(got - ref["S"])
    print(f"scatter {shape}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert np.array_equal(got, got.T)
    again = run_scatter(ref, extra_x=0, extra_y=0)
    assert np.array_equal(got, again)


# --------------------------------------------------------------------------------------------------------- class sums
def class_cases(N):
    """name -> codes [N] (-1: in no class), classes.  C of 1, 2, 37 and N; an empty run; rows left out."""
    rng = np.random.default_rng(N)
    cases = {"one class": (np.zeros(N, np.int64), 1), "every row its own class": (rng.permutation(N), N)}
    for C in (2, 37):
        if C <= N:
            codes = rng.integers(0, C, N)
            cases[f"{C} classes"] = (codes, C)
            holes = codes.copy()
            holes[holes == 1] = 0             # an empty run
            holes[rng.random(N) < 0.15] = -1  # rows of no class
            cases[f"{C} classes, one empty, rows left out"] = (holes, C)
    nobody = np.full(N, -1)
    nobody[N // 2] = min(1, N - 1)
    cases["one row listed"] = (nobody, min(2, N))
    return cases


@pytest.mark.parametrize("shape", shapes(), ids=SHAPE_IDS)
def test_class_sums_meet_their_bound(shape):
    ref = reference(*shape)
    X, mean = ref["X"], ref["mean"]
    N, D = X.shape
    for name, (codes, C) in class_cases(N).items():
        order, run_ptr, counts = P.runs_of(codes, C)
        for m in (mean, None):
            want, mags = P.class_sums(X, m, order, run_ptr)
            got = run_sums(X, m, order, run_ptr)
            assert (np.abs(got - want) <= N * 2.0 ** -52 * mags).all(), (name, m is None)
            assert not got[counts == 0].any(), name
        assert np.array_equal(got, run_sums(X, None, order, run_ptr, extra_x=0)), name


# --------------------------------------------------------------------------------------------------------- projection
@pytest.mark.parametrize("shape", shapes(), ids=SHAPE_IDS)
def test_projection_meets_its_bound(shape):
    ref = reference(*shape)
    X, mean = ref["X"], ref["mean"]
    N, D = X.shape
    rng = np.random.default_rng(D)
    for Pn in sorted({1, min(2, D), D}):
        comp = (rng.standard_normal((Pn, D)) / np.sqrt(D)).astype(np.float32)
        want, mags = P.projection(X, mean, comp)
        got = run_project(X, mean, comp)
        assert (np.abs(got - want) <= (D + 1) * U * mags).all(), Pn
        assert np.array_equal(got, run_project(X, mean, comp, extra_x=0, extra_s=0)), Pn


# ------------------------------------------------------------------------------------------------------ refused shapes
def test_refused_shapes_leave_everything_untouched():
    L, lib = _lib()
    N, D, M, C, Pn = 300, 70, 2, 5, 3
    ref = reference(N, D, M)
    wx, wy = wide_rows(ref["X"], 5), wide_rows(ref["Y"], 3)
    mean = dev(ref["full"])
    order, run_ptr, _ = P.runs_of(ref["cls"] % C, C)
    order_d, run_d = dev(order), dev(run_ptr)
    comp = dev(np.eye(Pn, D, dtype=np.float32))
    S = Padded((D + M) ** 2, torch.float64, -5.0)
    sums = Padded(C * D, torch.float64, -5.0)
    scores = Padded(N * Pn, torch.float32, -5.0)
    big = max(lib.mmvae_pca_scatter_workspace_bytes(N, D, M), lib.mmvae_pca_group_sums_workspace_bytes(N, D))
    ws = torch.full((big + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    st = _stream()
    x, y, mu, w = wx.data_ptr(), wy.data_ptr(), mean.data_ptr(), ws.data_ptr()
    ok_scatter = [N, D, x, D + 5, M, y, M + 3, mu, S.ptr(), w, big, st]
    bad_scatter = {"N 0": {0: 0}, "D 0": {1: 0}, "W 513": {1: 511, 3: 511}, "ldx < D": {3: D - 1}, "M 9": {4: 9, 6: 12},
                   "M < 0": {4: -1}, "ldy < M": {6: 1}, "null y": {5: None}, "null x": {2: None}, "null mean": {7: None},
                   "null out": {8: None}, "null workspace": {9: None},
                   "short workspace": {10: lib.mmvae_pca_scatter_workspace_bytes(N, D, M) - 16}, "odd workspace": {9: w + 8}}
    for what, change in bad_scatter.items():
        args = [change.get(i, a) for i, a in enumerate(ok_scatter)]
        assert lib.mmvae_pca_scatter_f32(*args) == L.ERR_ARG, what
    ok_sums = [N, D, x, D + 5, mu, C, order_d.data_ptr(), run_d.data_ptr(), sums.ptr(), w, big, st]
    bad_sums = {"N 0": {0: 0}, "D 0": {1: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: D - 1}, "C 0": {5: 0}, "C > N": {5: N + 1},
                "null x": {2: None}, "null order": {6: None}, "null run_ptr": {7: None}, "null out": {8: None},
                "null workspace": {9: None}, "short workspace": {10: lib.mmvae_pca_group_sums_workspace_bytes(N, D) - 16},
                "odd workspace": {9: w + 4}}
    for what, change in bad_sums.items():
        args = [change.get(i, a) for i, a in enumerate(ok_sums)]
        assert lib.mmvae_pca_group_sums_f64(*args) == L.ERR_ARG, what
    ok_project = [N, D, x, D + 5, mu, Pn, comp.data_ptr(), scores.ptr(), Pn, st]
    bad_project = {"N 0": {0: 0}, "D 0": {1: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: D - 1}, "P 0": {5: 0},
                   "P > D": {5: D + 1, 8: D + 1}, "lds < P": {8: Pn - 1}, "null x": {2: None}, "null mean": {4: None},
                   "null components": {6: None}, "null scores": {7: None}}
    for what, change in bad_project.items():
        args = [change.get(i, a) for i, a in enumerate(ok_project)]
        assert lib.mmvae_pca_project_f32(*args) == L.ERR_ARG, what
    torch.cuda.synchronize()
    assert S.untouched() and sums.untouched() and scores.untouched() and bool((ws == 0xAB).all())
    # ... and the same buffers take the calls as they stand
    for fn, args in ((lib.mmvae_pca_scatter_f32, ok_scatter), (lib.mmvae_pca_group_sums_f64, ok_sums),
                     (lib.mmvae_pca_project_f32, ok_project)):
        L.check(fn(*args), "the unchanged call")
    torch.cuda.synchronize()
    assert S.untouched_outside() and sums.untouched_outside() and scores.untouched_outside()
    assert not S.untouched() and not sums.untouched() and not scores.untouched()


# ---------------------------------------------------------------------------------------------------------- end to end
def _metadata(ref, seed=5):
    N = len(ref["X"])
    rng = np.random.default_rng(seed)
    species = np.array(["human", "mouse", "rat", "pig"], dtype=object)[ref["cls"] % 4]
    donor = np.array([f"d{i}" for i in rng.integers(0, 37, N)], dtype=object)
    donor[rng.random(N) < 0.1] = np.nan
    frame = pd.DataFrame({"species": species, "donor": donor})
    if ref["Y"] is not None:
        for m in range(ref["Y"].shape[1]):
            frame[f"y{m}"] = ref["Y"][:, m]
    return frame


@pytest.mark.parametrize("n_comps", [None, 7])
def test_pc_regression_equals_the_restatement_on_the_devices_moments(n_comps):
    from mmvae_amd import pca

    ref = reference(2100, 128, 3)
    X, N, D = ref["X"], 2100, 128
    meta = _metadata(ref)
    z = dev(X)
    covariates = ("species", "y0", "donor", "y1", "y2")  # (the numeric ones in the order of the reference's Y)
    out = pca.pc_regression(z, meta, covariates, n_comps)
    S = out.fit.scatter
    assert S.shape == (131, 131) and np.array_equal(S, S.T)
    assert np.array_equal(out.fit.mean.cpu().numpy(), ref["mean"]) and np.array_equal(out.fit.covariate_mean.cpu().numpy(),
                                                                                       ref["full"][D:])
    assert (np.abs(S - ref["S"]) <= (chain() + 2) * U * ref["T"]).all()
    assert out.summary["covariate"].tolist() == list(covariates) and out.summary["n_classes"].tolist() == [4, 0, 38, 0, 0]
    Pn = D if n_comps is None else n_comps
    assert out.summary["n_comps"].tolist() == [Pn] * 5 and len(out.per_component) == Pn
    for name in covariates:
        if name.startswith("y"):
            r2, r2var = P.from_moments(S, N, n_comps, cov=int(name[1]), n_features=D)
        else:
            codes = pd.factorize(meta[name], sort=True)[0]
            L = codes.max() + 1
            codes = np.where(codes < 0, L, codes)
            L = codes.max() + 1
            order, run_ptr, counts = P.runs_of(codes, L)
            sums = pca.group_sums(z, dev(order), dev(run_ptr), out.fit.mean).cpu().numpy()
            want, mags = P.class_sums(X, ref["mean"], order, run_ptr)
            assert (np.abs(sums - want) <= N * 2.0 ** -52 * mags).all()
            r2, r2var = P.from_moments(S, N, n_comps, sums, counts)
        got = out.per_component[f"r2.{name}"].to_numpy()
        assert (np.abs(got - r2) <= 1e-12).all() and abs(out.pcr(name) - r2var) <= 1e-12, name
        assert 0.0 <= r2var <= 1.0


def test_full_rank_pcr_is_the_trace_ratio():
    from mmvae_amd import pca

    ref = reference(2100, 128, 3)
    X, N, D = ref["X"], 2100, 128
    meta = _metadata(ref)
    out = pca.pc_regression(dev(X), meta, ("species", "donor"))
    for name in ("species", "donor"):
        codes = pd.factorize(meta[name], sort=True)[0]
        codes = np.where(codes < 0, codes.max() + 1, codes)
        order, run_ptr, counts = P.runs_of(codes, codes.max() + 1)
        sums, _ = P.class_sums(X, ref["mean"], order, run_ptr)
        want = ((sums ** 2).sum(1) / counts).sum() / np.trace(ref["S"][:D, :D])
        got = out.pcr(name)
        print(f"full-rank pcr {name}: {got:.15f} against {want:.15f}")
        assert abs(got - want) <= 2 * (chain() + 2) * U * want, name


def test_score_variances_are_the_explained_variances():
    from mmvae_amd import pca

    ref = reference(1030, 130, 0)
    X, N, D = ref["X"], 1030, 130
    z = wide_rows(X, 5)[:, :D]
    fit = pca.pca_fit(z)
    scores = pca.pca_transform(fit, z).cpu().numpy().astype(np.float64)
    assert scores.shape == (N, D) and fit.components.shape == (D, D)
    V = fit.components64
    assert np.array_equal(fit.mean.cpu().numpy(), ref["mean"])
    assert np.array_equal(fit.components.cpu().numpy(), V.astype(np.float32))
    s64, mags = P.projection(X, ref["mean"], V.astype(np.float32))
    b = (D + 2) * U * mags
    tol = (2 * np.abs(s64) * b + b * b).sum(0) + (chain() + 2) * U * np.einsum("pu,uv,pv->p", np.abs(V), ref["T"], np.abs(V)) \
        + D * 2.0 ** -52 * fit.eigenvalues[0]
    got = (scores ** 2).sum(0)
    print(f"variances: largest error / tolerance = {(np.abs(got - fit.eigenvalues) / tol).max():.3f}")
    assert (np.abs(got - fit.eigenvalues) <= tol).all()
    assert (np.abs(got / (N - 1) - fit.explained_variance) <= tol / (N - 1)).all()
    assert abs(fit.explained_variance_ratio.sum() - 1.0) <= 1e-14 and (np.diff(fit.eigenvalues) <= 0).all()
    two = pca.pca_embeddings(z)
    assert two.shape == (N, 2) and torch.equal(two, pca.pca_transform(pca.pca_fit(z, 2), z))
