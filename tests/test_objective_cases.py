"""The exact-sum cases of tests/objective_cases.py do what tests/test_objective_kernels_gpu.py relies on (no GPU):
 * their fp32 sums do not depend on the summation order, and no cell's softmax is one-hot;
 * an fp32 kernel that normalises the weights by the sum (w = ex / sum) meets the w tolerances against fp64, so a correct
   kernel can pass;
 * the formula the kernels used before (w = expf(v - lse)) does not meet them at SE ~ 1e4, so the tests discriminate."""
import numpy as np
import pytest

from tests import objective_cases as OC

MULTI_K = [c for c in OC.FINALIZE_CASES if c[1] > 1]


def _exact(B, K, T):
    return OC.se_parts_exact(B, K, T, OC.EXACT_LEVEL, OC.exact_seed(B, K, T))


def _pairwise_f32(a):
    a = np.asarray(a, np.float32)
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros_like(a[:1])])
        a = (a[0::2] + a[1::2]).astype(np.float32)
    return a[0]


def _seq_f32(a):
    s = np.zeros_like(a[0])
    for row in a:
        s = (s + row).astype(np.float32)
    return s


@pytest.mark.parametrize("B,K,T", OC.FINALIZE_CASES)
def test_exact_parts_are_order_independent(B, K, T):
    p = _exact(B, K, T)
    assert p.dtype == np.float32 and p.shape == (T, K * B) and p.min() >= 0
    assert np.array_equal(p * 64, np.rint(p * 64)), "every partial is a multiple of 1/64"
    fwd, rev, pair = _seq_f32(p), _seq_f32(p[::-1]), _pairwise_f32(p)
    assert np.array_equal(fwd, rev) and np.array_equal(fwd, pair)
    assert np.array_equal(fwd.astype(np.float64), p.astype(np.float64).sum(0)), "the fp32 total is the exact total"
    tot = fwd.reshape(K, B)
    assert tot.max() < 2 ** 14 and abs(np.median(tot) / OC.EXACT_LEVEL - 1) < 0.03
    assert (tot.max(0) - tot.min(0)).max() <= 4.0


def _exact_logweights(B, K, T, iwae):
    """fp32 log-weights [K, B] of an exact-sum case (exact in fp32) and the fp64 reference weights."""
    p = _exact(B, K, T)
    se = _seq_f32(p).reshape(K, B)
    if not iwae:
        return -se, OC.elbo_ref(p, None, None, B, K, 0, 1.0)[1]
    r = OC.logratio_even(B, K, 7)
    c = np.float32(1.0) / np.float32(B)
    v = (-se - c * r).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), -se.astype(np.float64) - (1.0 / B) * r.astype(np.float64))
    return v, OC.iwae_ref(p, r, None, B, K, 0, 1.0)[1]


IWAE_EXACT = [OC.PRODUCTION_CASE + (True,)]


@pytest.mark.parametrize("B,K,T,iwae", [c + (False,) for c in MULTI_K] + IWAE_EXACT)
def test_no_exact_case_is_one_hot(B, K, T, iwae):
    _, w_ref = _exact_logweights(B, K, T, iwae)
    assert w_ref.reshape(K, B).max(0).max() <= 0.999


@pytest.mark.parametrize("B,K,T,iwae", [c + (False,) for c in MULTI_K] + IWAE_EXACT)
def test_ratio_form_meets_the_w_bounds_and_lse_form_does_not(B, K, T, iwae):
    v, w_ref = _exact_logweights(B, K, T, iwae)
    good, bad = OC.w_ratio_form_f32(v), OC.w_lse_form_f32(v)
    ok, worst = OC.w_close(good, w_ref, **OC.W_EXACT_TOL)
    dsum = np.abs(good.astype(np.float64).sum(0) - 1).max()
    print(f"ex/sum: worst |dw| / tol {worst:.3g}, max |sum_k w - 1| {dsum:.3g}")
    assert ok and dsum <= OC.W_SUM_TOL
    ok_bad, worst_bad = OC.w_close(bad, w_ref, **OC.W_EXACT_TOL)
    dsum_bad = np.abs(bad.astype(np.float64).sum(0) - 1).max()
    print(f"expf(v - lse): worst |dw| / tol {worst_bad:.3g}, max |sum_k w - 1| {dsum_bad:.3g}")
    assert not ok_bad and dsum_bad > OC.W_SUM_TOL


def test_k1_weights_are_one():
    B, K, T = 513, 1, 125
    out6, w, recon_row = OC.elbo_ref(_exact(B, K, T), None, None, B, K, 0, 1.0)
    assert np.array_equal(w, np.ones(B)) and out6[1] == recon_row.sum()


def test_references_agree_with_the_oracle():
    """elbo_ref / iwae_ref / logratio_ref against oracle.mmvae_oracle.elbo / elbo_iwae in fp64 on a small model-free case
    (xhat = x + residual, so SE is the residual's squared norm, split over T tiles)."""
    import torch

    from oracle import mmvae_oracle as O

    B, K, Z, G, T, klw = 6, 3, 5, 12, 4, 0.7
    tol = 1e-6  # the oracle takes log(K) in fp32: B * 3e-8
    g = torch.Generator().manual_seed(3)
    mu, a = torch.randn(B, Z, generator=g), torch.randn(B, Z, generator=g) * 0.5
    std = (a.exp() + 1e-4).sqrt()
    eps = torch.randn(K, B, Z, generator=g)
    z = mu + std * eps
    x = torch.randn(B, G, generator=g)
    d = lambda t: t.double()  # noqa: E731
    stat = torch.stack([mu.sum(1), (std * std).sum(1)]).numpy()
    res = torch.randn(K, B, G, generator=g)
    xhat = (x.unsqueeze(0) + res).reshape(K * B, G)
    se_part = (d(xhat).reshape(K, B, T, G // T) - d(x).reshape(1, B, T, G // T)).pow(2).sum(-1).permute(2, 0, 1).reshape(T, K * B)
    se_part = se_part.numpy()
    want = O.elbo(d(mu), d(std), d(x), d(xhat), float(np.float32(klw)), K)
    kl_row = (0.5 * (d(std)**2 + d(mu)**2 - 1 - (d(std)**2).log())).sum(-1).numpy()
    out6, w, _ = OC.elbo_ref(se_part, kl_row, stat, B, K, Z, klw)
    assert abs(out6[0] - float(want["loss"])) < tol and abs(out6[1] - float(want["recon_loss"])) < tol
    assert abs(out6[2] - float(want["kl_loss"])) < 1e-9 and abs(w.reshape(K, B).sum(0) - 1).max() < 1e-12
    r, mag = OC.logratio_ref(std.numpy(), eps.numpy(), z.numpy())
    assert (mag >= np.abs(r)).all()
    want = O.elbo_iwae(d(mu), d(std), d(x), d(xhat), float(np.float32(klw)), K, d(eps), d(z))
    out6, w, rows3 = OC.iwae_ref(se_part, r, stat, B, K, Z, klw)
    assert abs(out6[0] - float(want["loss"])) < tol and abs(out6[1] - float(want["recon_loss"])) < tol
    assert abs(out6[2] - float(want["kl_loss"])) < 1e-9
    assert abs(out6[4] - float(mu.double().mean())) < 1e-6 and abs(out6[5] - float((std.double() ** 2).mean())) < 1e-6
