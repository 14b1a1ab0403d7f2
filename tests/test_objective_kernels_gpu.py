"""Direct tests of the objective kernels (mmvae_amd/csrc/elbo_optim.hip) against fp64 at the shapes the training step runs
them at: mmvae_elbo_finalize, mmvae_iwae_logratio, mmvae_elbo_finalize_iwae, mmvae_iwae_bwd_terms (the last three through
the C-ABI, they have no ops wrapper), the latent chain of the full-IWAE program against torch autograd, and the argument
combinations of mmvae_reparam_kl_bwd / mmvae_mse_sum_fwd_bwd that program uses.  Inputs and references:
tests/objective_cases.py (tests/test_objective_cases.py shows on the CPU that an fp32 kernel can meet the w bounds).

Tolerances.  Scalars of out6: those of test_kernels_gpu.test_elbo_finalize (1e-5 of the reconstruction term on loss and
recon, 1e-6 on kl and the statistics).  Per-cell bound: 1e-6 relative.  Weights: rtol 1e-5 / atol 1e-7 on the exact-sum
cases (SE ~ 1e4, every fp32 sum exact), and sum_k w within 1e-5 of 1; rtol 1e-4 / atol 1e-6 on the random cases (SE ~ 30,
whose fp32 sums carry ~2e-6).  Log-ratio: 2e-6 of sum_j |term_j| (a wavefront sum of Z one-ulp terms stays under ~12 fp32
eps of that).  Gradients: rel-L2 1e-6 for the elementwise terms, 1e-5 through the chain (test_reparam_kl's bound)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import objective_cases as OC  # noqa: E402
from tests.helpers import rel_l2  # noqa: E402

KLW = 0.8


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from mmvae_amd import _lib, ops as _ops

    assert _lib.load().mmvae_abi_version() >= 3
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from mmvae_amd import _lib

    return _lib.load()


def dev(a):
    return (torch.tensor(a) if isinstance(a, np.ndarray) else a).cuda()  # a copy: the cases are read-only


def host(t):
    return t.detach().cpu().double().numpy()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _empty(*shape):
    return torch.empty(*shape, dtype=torch.float32, device="cuda")


def _se_parts(kind, B, K, T):
    if kind == "exact":
        return OC.se_parts_exact(B, K, T, OC.EXACT_LEVEL, OC.exact_seed(B, K, T))
    return OC.se_parts_random(B, K, T, OC.RANDOM_LEVEL, OC.exact_seed(B, K, T) + 1)


def _rel(got, want, scale=None):
    return abs(float(got) - float(want)) / abs(float(want if scale is None else scale))


def _check_w(kind, w, w_ref, K, B):
    tol = OC.W_EXACT_TOL if kind == "exact" else OC.W_RANDOM_TOL
    ok, worst = OC.w_close(w, w_ref, **tol)
    dsum = np.abs(w.reshape(K, B).sum(0) - 1).max()
    print(f"w: worst |dw| / (atol + rtol |w|) = {worst:.3g} at {tol}; max |sum_k w - 1| = {dsum:.3g}")
    assert ok, f"w off by {worst:.3g} x the tolerance {tol}"
    if kind == "exact":
        assert dsum <= OC.W_SUM_TOL


def _check_stats_words(o, ref):
    assert abs(o[4] - ref[4]) < 1e-6 and abs(o[5] - ref[5]) < 1e-6


# ------------------------------------------------------------------------------------------ a. mmvae_elbo_finalize
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("B,K,T", OC.FINALIZE_CASES)
def test_elbo_finalize_shapes(ops, lib, B, K, T, kind):
    from mmvae_amd import _lib

    Z = OC.Z_STATS
    se_part = _se_parts(kind, B, K, T)
    kl_row, stat = OC.kl_and_stats(B, Z, 5)
    ref6, w_ref, recon_ref = OC.elbo_ref(se_part, kl_row, stat, B, K, Z, KLW)
    sp, kl, st = dev(se_part), dev(kl_row), dev(stat)
    out_h, w_h = ops.elbo_finalize(sp, kl, st, B=B, K=K, Z=Z, kl_weight=KLW, want_w=True)
    klw_dev = torch.tensor([KLW], device="cuda")
    out_d, w_d = ops.elbo_finalize(sp, kl, st, B=B, K=K, Z=Z, kl_weight_dev=klw_dev, want_w=True)
    assert torch.equal(out_h, out_d) and torch.equal(w_h, w_d)
    # the same entry point through the C-ABI, to see the per-cell bound (ops keeps recon_row to itself)
    out_c, w_c, recon_row = _empty(6), _empty(K * B), _empty(B)
    _lib.check(lib.mmvae_elbo_finalize(B, K, T, _p(sp), _p(kl), _p(st), Z, None, KLW, _p(out_c), _p(w_c), _p(recon_row),
                                       _st()), "mmvae_elbo_finalize")
    assert torch.equal(out_c, out_h) and torch.equal(w_c, w_h)
    o, w, rr = host(out_h), host(w_h), host(recon_row)
    recon = ref6[1]
    print(f"B={B} K={K} T={T} {kind}: loss {_rel(o[0], ref6[0], recon):.3g} recon {_rel(o[1], recon):.3g} "
          f"kl {_rel(o[2], ref6[2]):.3g} recon_row {np.abs(rr / recon_ref - 1).max():.3g}")
    assert _rel(o[1], recon) <= 1e-5
    assert _rel(o[2], ref6[2]) <= 1e-6
    assert _rel(o[0], ref6[0], recon) <= 1e-5
    assert abs(o[3] - KLW) < 1e-7
    _check_stats_words(o, ref6)
    assert (np.abs(rr - recon_ref) <= 1e-6 * np.abs(recon_ref)).all()
    _check_w(kind, w, w_ref, K, B)


def test_objective_entry_points_reject_k_above_maxk(ops, lib):
    from mmvae_amd import _lib

    B, K = 4, 65
    sp = torch.ones(1, K * B, device="cuda")
    with pytest.raises(_lib.HipLibraryError, match="MMVAE_ERR_ARG"):
        ops.elbo_finalize(sp, None, None, B=B, K=K, want_w=True)
    out6, w, rows3, r = _empty(6), _empty(K * B), _empty(3, B), torch.zeros(K, B, device="cuda")
    assert lib.mmvae_elbo_finalize_iwae(B, K, 1, _p(sp), _p(r), None, 0, None, 1.0, _p(out6), _p(w), _p(rows3),
                                        _st()) == _lib.ERR_ARG
    std, ez = torch.ones(B, 8, device="cuda"), torch.zeros(K, B, 8, device="cuda")
    assert lib.mmvae_iwae_logratio(B, 8, K, _p(std), _p(ez), _p(ez), _p(r), _st()) == _lib.ERR_ARG


# ------------------------------------------------------------------------------------------ b. mmvae_iwae_logratio
def _logratio(lib, std, eps, z):
    from mmvae_amd import _lib

    K, B, Z = eps.shape
    out = _empty(K, B)
    _lib.check(lib.mmvae_iwae_logratio(B, Z, K, _p(std), _p(eps), _p(z), _p(out), _st()), "mmvae_iwae_logratio")
    return out


@pytest.mark.parametrize("K,B,Z", [(3, 33, 8), (1, 7, 64), (5, 33, 65), (64, 5, 128), (10, 64, 200)])
def test_iwae_logratio(lib, K, B, Z):
    std, eps, z = OC.logratio_inputs(K, B, Z, 11)
    assert std.min() >= 0.05 and std.max() <= 3.0
    r_ref, mag = OC.logratio_ref(std, eps, z)
    r = host(_logratio(lib, dev(std), dev(eps), dev(z)))
    print(f"K={K} B={B} Z={Z}: max |r - r_ref| / sum_j |term_j| = {(np.abs(r - r_ref) / mag).max():.3g}")
    assert (np.abs(r - r_ref) <= 2e-6 * mag).all()


# ------------------------------------------------------------------------------------- c. mmvae_elbo_finalize_iwae
def _finalize_iwae(lib, se_part, r, stat, B, K, Z, klw_dev, klw_host):
    from mmvae_amd import _lib

    T = se_part.shape[0]
    out6, w, rows3 = _empty(6), _empty(K * B), _empty(3, B)
    _lib.check(lib.mmvae_elbo_finalize_iwae(B, K, T, _p(se_part), _p(r), _p(stat), Z, _p(klw_dev), klw_host, _p(out6), _p(w),
                                            _p(rows3), _st()), "mmvae_elbo_finalize_iwae")
    return out6, w, rows3


def _check_iwae(lib, kind, B, K, T, r, klw, weight_on_device):
    Z = OC.Z_STATS
    se_part = _se_parts(kind, B, K, T)
    _, stat = OC.kl_and_stats(B, Z, 5)
    ref6, w_ref, rows_ref = OC.iwae_ref(se_part, r, stat, B, K, Z, klw)
    klw_dev = torch.tensor([klw], device="cuda") if weight_on_device else None
    out6, w, rows3 = _finalize_iwae(lib, dev(se_part), dev(r), dev(stat), B, K, Z, klw_dev, 1.0 if weight_on_device else klw)
    o, w, rows = host(out6), host(w), host(rows3)
    w_abs_se = (w_ref.reshape(K, B) * np.asarray(se_part, np.float64).sum(0).reshape(K, B)).sum(0)
    w_abs_r = (w_ref.reshape(K, B) * np.abs(np.asarray(r, np.float64))).sum(0)
    print(f"B={B} K={K} T={T} {kind} klw={klw}: bound {np.abs(rows[0] / rows_ref[0] - 1).max():.3g} "
          f"wse {(np.abs(rows[1] - rows_ref[1]) / w_abs_se).max():.3g} wr {(np.abs(rows[2] - rows_ref[2]) / w_abs_r).max():.3g}")
    assert (np.abs(rows[0] - rows_ref[0]) <= 1e-6 * np.abs(rows_ref[0])).all()
    assert (np.abs(rows[1] - rows_ref[1]) <= 1e-5 * w_abs_se).all()
    assert (np.abs(rows[2] - rows_ref[2]) <= 1e-5 * w_abs_r).all()
    _check_w(kind, w, w_ref, K, B)
    # scalars: against fp64 to the bounds of their rows, and against the kernel's own rows to an fp32 rounding
    assert _rel(o[0], ref6[0]) <= 1e-5
    assert _rel(o[1], ref6[1], w_abs_se.sum()) <= 1e-5
    assert _rel(o[2], ref6[2], w_abs_r.mean()) <= 1e-5
    assert o[3] == float(np.float32(klw))
    _check_stats_words(o, ref6)
    ulp = 2.0 ** -23
    assert _rel(o[0], rows[0].sum()) <= ulp and _rel(o[1], rows[1].sum()) <= ulp
    assert _rel(o[2], rows[2].mean(), np.abs(rows[2]).mean()) <= ulp


@pytest.mark.parametrize("klw,weight_on_device", [(0.7, True), (1.0, False)])
@pytest.mark.parametrize("B,K,T", OC.FINALIZE_CASES)
def test_elbo_finalize_iwae_shapes(lib, B, K, T, klw, weight_on_device):
    _check_iwae(lib, "random", B, K, T, OC.logratio_random(B, K, 7), klw, weight_on_device)


def test_elbo_finalize_iwae_production_exact(lib):
    """SE ~ 1e4 with exact sums, r even integers and c = 2^-9: the log-weights are exact in fp32 (fma or not), so w is
    held to the exact-case tolerances."""
    B, K, T = OC.PRODUCTION_CASE
    _check_iwae(lib, "exact", B, K, T, OC.logratio_even(B, K, 7), 1.0, False)


# ----------------------------------------------------------------------------------------- d. mmvae_iwae_bwd_terms
def _bwd_terms(lib, w, z, std, dz, dstd, klw_dev, klw_host):
    from mmvae_amd import _lib

    K, B, Z = z.shape
    _lib.check(lib.mmvae_iwae_bwd_terms(B, Z, K, _p(klw_dev), klw_host, _p(w), _p(z), _p(std), _p(dz), _p(dstd), _st()),
               "mmvae_iwae_bwd_terms")


@pytest.mark.parametrize("K,B,Z", [(5, 520, 256), (3, 33, 10)])  # the first is more than one pass of the 2048 x 256 grid
def test_iwae_bwd_terms(lib, K, B, Z):
    klw, pad = 0.7, 64
    std, _, z = OC.logratio_inputs(K, B, Z, 13)
    rng = np.random.default_rng(17)
    w = rng.uniform(0.05, 1.0, size=(K, B))
    w = (w / w.sum(0)).astype(np.float32)
    dz0 = rng.standard_normal((K, B, Z)).astype(np.float32)
    c = float(np.float32(klw)) / B
    dz_ref = dz0.astype(np.float64) + c * w.astype(np.float64)[:, :, None] * z.astype(np.float64)
    dstd_ref = -c / std.astype(np.float64)
    dz = dev(dz0)
    dstd = torch.full((B * Z + pad,), float("nan"), device="cuda")  # every (b, j) written; nothing past the end
    _bwd_terms(lib, dev(w), dev(z), dev(std), dz, dstd, torch.tensor([klw], device="cuda"), 1.0)
    got = dstd.cpu()
    assert torch.isfinite(got[:B * Z]).all() and torch.isnan(got[B * Z:]).all()
    assert rel_l2(dz, torch.from_numpy(dz_ref)) < 1e-6
    assert rel_l2(got[:B * Z].reshape(B, Z), torch.from_numpy(dstd_ref)) < 1e-6
    # written once: a second launch on the result leaves dstd_extra as it is and adds the same term to dz again
    first = got.clone()
    _bwd_terms(lib, dev(w), dev(z), dev(std), dz, dstd, None, klw)
    assert rel_l2(dstd.cpu()[:B * Z], first[:B * Z]) < 1e-6
    assert rel_l2(dz, torch.from_numpy(2 * dz_ref - dz0.astype(np.float64))) < 1e-6


# --------------------------------------------------------------------------------- e. latent chain against autograd
@pytest.mark.parametrize("B,Z,K", [(33, 10, 4), (64, 128, 10)])
def test_iwae_latent_chain_matches_autograd(ops, lib, B, Z, K):
    """L(mu, a) = sum_b -logmeanexp_k(-SE_kb - c r_kb), SE_kb = <q_kb, z_kb> + 30, c = 0.7 / B: the kernels of the
    full-IWAE program from the encoder heads to their gradients, in the engine's order, with the decoder replaced by a
    linear SE.  Pins the signs and the klw / B scaling of logratio, finalize_iwae and bwd_terms."""
    klw, var_eps = 0.7, 1e-4
    g = torch.Generator().manual_seed(100 + Z)
    mu = torch.randn(B, Z, generator=g)
    a = torch.randn(B, Z, generator=g) * 0.5
    eps = torch.randn(K, B, Z, generator=g)
    q = torch.randn(K, B, Z, generator=g) / Z ** 0.5  # SE_kb spread by O(1) over k: the softmax is not one-hot
    c = float(np.float32(klw)) / B

    mu64, a64 = mu.double().requires_grad_(True), a.double().requires_grad_(True)
    std64 = (a64.exp() + var_eps).sqrt()
    z64 = mu64 + std64 * eps.double()
    r64 = (-std64.log().unsqueeze(0) - 0.5 * eps.double() ** 2 + 0.5 * z64 ** 2).sum(-1)
    se64 = (q.double() * z64).sum(-1) + 30.0
    loss = (-(torch.logsumexp(-se64 - c * r64, 0) - np.log(K))).sum()
    loss.backward()

    mu_d, eps_d, q_d = dev(mu), dev(eps), dev(q)
    std, z, _, stat = ops.reparam_kl_fwd(mu_d, dev(a), eps_d, var_eps=var_eps)
    r = _logratio(lib, std, eps_d, z)
    se = ((q.double() * z.cpu().double()).sum(-1) + 30.0).float().reshape(1, K * B)  # SE from the kernel's z, T = 1
    out6, w, rows3 = _finalize_iwae(lib, dev(se), r, stat, B, K, Z, torch.tensor([klw], device="cuda"), 1.0)
    assert _rel(out6[0], loss.detach()) <= 1e-5
    dz = (w.reshape(K, B, 1) * q_d).contiguous()
    dstd = _empty(B, Z)
    _bwd_terms(lib, w, z, std, dz, dstd, torch.tensor([klw], device="cuda"), 1.0)
    dmu, da = ops.reparam_kl_bwd(mu_d, std, eps_d, dz, dstd_extra=dstd, kl_scale=0.0, var_eps=var_eps)
    print(f"B={B} Z={Z} K={K}: dmu {rel_l2(dmu, mu64.grad):.3g} da {rel_l2(da, a64.grad):.3g}")
    assert rel_l2(dmu, mu64.grad) < 1e-5
    assert rel_l2(da, a64.grad) < 1e-5


# --------------------------------------------------------------------------------------------- f. reparam_kl gaps
@pytest.mark.parametrize("Z", [1, 63, 64, 65])
def test_reparam_kl_extras_without_dz(ops, Z):
    """Z around the wavefront width, a_raw over [-8, 4] (variance from var_eps-dominated to e^4), and the backward with
    dmu_extra and dstd_extra but no dz: the arguments of the full-IWAE program."""
    B, K, var_eps, scale = 5, 2, 1e-4, 0.37
    g = torch.Generator().manual_seed(Z)
    mu = torch.randn(B, Z, generator=g)
    a = torch.rand(B, Z, generator=g) * 12 - 8
    a.view(-1)[0], a.view(-1)[-1] = -8.0, 4.0
    eps = torch.randn(K, B, Z, generator=g)
    gmu, gstd, gkl = torch.randn(B, Z, generator=g), torch.randn(B, Z, generator=g), torch.randn(B, generator=g)
    mu64, a64 = mu.double().requires_grad_(True), a.double().requires_grad_(True)
    var = a64.exp() + var_eps
    std = var.sqrt()
    klr = (0.5 * (var + mu64 ** 2 - 1 - var.log())).sum(-1)
    ((mu64 * gmu.double()).sum() + (std * gstd.double()).sum() + scale * (klr * gkl.double()).sum()).backward()
    sd, zd, kl_row, stat = ops.reparam_kl_fwd(dev(mu), dev(a), dev(eps), var_eps=var_eps)
    z = mu.double() + std.detach() * eps.double()
    torch.testing.assert_close(zd.cpu().double(), z, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(sd.cpu().double(), std.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(kl_row.cpu().double(), klr.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(stat.cpu().double()[0], mu.double().sum(1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(stat.cpu().double()[1], var.detach().sum(1), rtol=1e-5, atol=1e-5)
    dmu, da = ops.reparam_kl_bwd(dev(mu), sd, None, None, dmu_extra=dev(gmu), dstd_extra=dev(gstd), dkl_row=dev(gkl),
                                 kl_scale=scale, var_eps=var_eps)
    assert rel_l2(dmu, mu64.grad) < 1e-5
    assert rel_l2(da, a64.grad) < 1e-5
    # kl_scale = 0 leaves the extras alone: dmu = dmu_extra, da = dstd_extra / (2 s) * (v - var_eps)
    dmu0, da0 = ops.reparam_kl_bwd(dev(mu), sd, None, None, dmu_extra=dev(gmu), dstd_extra=dev(gstd), dkl_row=dev(gkl),
                                   kl_scale=0.0, var_eps=var_eps)
    assert torch.equal(dmu0.cpu(), gmu)
    assert rel_l2(da0, gstd.double() / (2 * std.detach()) * a64.detach().exp()) < 1e-5


# ------------------------------------------------------------------------------------------ g. mse_sum_fwd_bwd gaps
@pytest.mark.parametrize("B,G", [(3, 1), (3, 255), (3, 256), (3, 257), (3, 20000)])
def test_mse_sum_strided_operands(ops, B, G):
    """G below, at and across the 256-thread strip; xhat and x are column slices of wider buffers (ld != G)."""
    g = torch.Generator().manual_seed(G)
    xh_w, x_w = torch.randn(B, G + 7, generator=g).cuda(), torch.randn(B, G + 5, generator=g).cuda()
    xhat, x = xh_w[:, 3:3 + G], x_w[:, 2:2 + G]
    assert xhat.stride(0) != G and x.stride(0) != G and xhat.stride(0) != x.stride(0)
    d = xhat.cpu().double() - x.cpu().double()
    se_ref = (d * d).sum(1)
    se, dx = ops.mse_sum_fwd_bwd(xhat, x, gscale=0.5)
    assert dx.shape == (B, G) and dx.is_contiguous()
    assert rel_l2(se, se_ref) < 1e-6
    assert rel_l2(dx, d) < 1e-6  # 0.5 * 2 d
    se2, none = ops.mse_sum_fwd_bwd(xhat, x, want_grad=False)
    assert none is None and torch.equal(se2, se)
    se3, dx3 = ops.mse_sum_fwd_bwd(xhat, x, gscale=0.5, gscale_dev=torch.tensor([-3.0], device="cuda"))
    assert torch.equal(se3, se)
    assert rel_l2(dx3, -3.0 * d) < 1e-6
