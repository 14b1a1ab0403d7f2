"""Inputs and fp64 references for the direct tests of the objective kernels (mmvae_elbo_finalize, mmvae_iwae_logratio,
mmvae_elbo_finalize_iwae, mmvae_iwae_bwd_terms; mmvae_amd/csrc/elbo_optim.hip).  numpy and CPU torch only: the CPU test
tests/test_objective_cases.py and the GPU test tests/test_objective_kernels_gpu.py share what is built here.  Every
builder is cached and hands out read-only arrays, so a reference is computed once.

Two kinds of squared-error partials se_part [T, K*B] (one row per column tile of the reconstruction, sample-major):
 * se_parts_exact: multiples of 1/64 whose per-(k, b) totals stay below 2^14, so a total needs fewer than 24 bits and every
   fp32 summation order gives the same, exact, total.  At a production-sized total (~1e4 for 20000 genes) an fp32 sum of
   ordinary numbers is rounded by ~1e-3, which moves a softmax weight by as much as the defect these cases are for
   (w = expf(v - lse) with lse rounded to an fp32 ulp of ~1e-3).  With exact sums, any error in w is the softmax's own.
 * se_parts_random: ordinary random numbers at small totals (<= 50), where fp32 sums are accurate to ~1e-6.

All references are computed in fp64 from the fp32 inputs."""
import functools

import numpy as np

# (B, K, T) of the finalisation tests: the small shape of test_kernels_gpu.test_elbo_finalize; reduce stride (B > 256),
# partial last workgroup (261 = 65 * 4 + 1) and three tile strides (T = 157 = recon tiles of 20000 genes in bf16x3 mode);
# the K = 1 path at T = 125 (the other modes' tile count); K = ELBO_MAXK with T one past a wavefront; a single tile;
# production.
FINALIZE_CASES = [(37, 3, 5), (261, 10, 157), (513, 1, 125), (5, 64, 65), (33, 5, 1), (512, 10, 157)]
PRODUCTION_CASE = (512, 10, 157)
EXACT_LEVEL = 1.0e4   # SE of a cell of 20000 genes
RANDOM_LEVEL = 30.0
Z_STATS = 128
# w against fp64: the elementwise tolerance of tests/test_kernels_gpu.py on the exact-sum cases, the tolerance of
# test_elbo_finalize on the random ones (their fp32 sums and log-weights carry ~2e-6 of their own)
W_EXACT_TOL = dict(rtol=1e-5, atol=1e-7)
W_RANDOM_TOL = dict(rtol=1e-4, atol=1e-6)
W_SUM_TOL = 1e-5


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def se_parts_exact(B, K, T, level, seed):
    """fp32 [T, K*B], non-negative multiples of 1/64.  The total of cell b, sample k is base_b + d_kb with base_b within
    2 % of `level` and d_kb in [0, 4] (softmax away from one-hot); the total is split at random over the T tiles."""
    assert level <= 1.6e4, "a total must stay below 2^14 (24 bits with the 6 fraction bits)"
    rng = np.random.default_rng(seed)
    base = np.rint(level * 64 * (1.0 + rng.uniform(-0.02, 0.02, size=B))).astype(np.int64)  # in units of 1/64
    d = rng.integers(0, 4 * 64 + 1, size=(K, B))
    total = (base[None, :] + d).reshape(K * B)
    assert total.max() < (1 << 14) * 64
    share = rng.uniform(0.2, 1.0, size=(T, K * B))
    parts = np.floor(total[None, :] * (share / share.sum(0))).astype(np.int64)
    rest = total - parts.sum(0)  # 0 <= rest <= T: goes to one random tile of the column
    assert rest.min() >= 0
    parts[rng.integers(0, T, size=K * B), np.arange(K * B)] += rest
    assert parts.min() >= 0 and np.array_equal(parts.sum(0), total)
    return _ro((parts / 64.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def se_parts_random(B, K, T, level, seed):
    """fp32 [T, K*B] ordinary non-negative random partials; per-(k, b) totals near `level` (<= 50)."""
    assert level <= 50
    rng = np.random.default_rng(seed)
    return _ro(np.abs((level / T) * (1.0 + 0.3 * rng.standard_normal((T, K * B)))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def kl_and_stats(B, Z, seed):
    """(kl_row [B], stat [2, B]) fp32 as mmvae_reparam_kl_fwd leaves them for a latent of width Z: per-cell KL, and the
    per-cell sums of mu and of the variance."""
    rng = np.random.default_rng(seed)
    kl_row = np.abs(rng.standard_normal(B) * 0.2 * Z).astype(np.float32)
    stat = np.stack([rng.standard_normal(B) * np.sqrt(Z), Z * rng.uniform(0.5, 1.5, size=B)]).astype(np.float32)
    return _ro(kl_row, stat)


@functools.lru_cache(maxsize=None)
def logratio_random(B, K, seed):
    """fp32 [K, B] ~ N(20, 10): the magnitude of r at Z = 128."""
    rng = np.random.default_rng(seed)
    return _ro((20.0 + 10.0 * rng.standard_normal((K, B))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def logratio_even(B, K, seed):
    """fp32 [K, B] even integers in [-60, 60]: with c = 2^-9 (kl weight 1, B = 512) c * r is a multiple of 2^-8, and
    -SE - c r of an exact-sum case is exact in fp32 with or without fma."""
    rng = np.random.default_rng(seed)
    return _ro((2 * rng.integers(-30, 31, size=(K, B))).astype(np.float32))


def _logsumexp0(v):
    mx = v.max(0)
    return mx + np.log(np.exp(v - mx).sum(0))


def _softmax0(v):
    e = np.exp(v - v.max(0))
    return e / e.sum(0)


def _stats_words(stat, B, Z):
    if stat is None:
        return 0.0, 0.0
    s = np.asarray(stat, np.float64)
    return s[0].sum() / (B * max(Z, 1)), s[1].sum() / (B * max(Z, 1))


def elbo_ref(se_part, kl_row, stat, B, K, Z, klw):
    """fp64 (out6, w [K*B], recon_row [B]) of mmvae_elbo_finalize: recon_b = SE_b (K = 1) or -logmeanexp_k(-SE_kb),
    w = softmax_k(-SE); out6 = loss, recon, kl (mean_b), kl weight, mean(mu), mean(var)."""
    se = np.asarray(se_part, np.float64).sum(0).reshape(K, B)
    if K == 1:
        recon_row, w = se[0].copy(), np.ones(B)
    else:
        recon_row = -(_logsumexp0(-se) - np.log(K))
        w = _softmax0(-se).reshape(-1)
    recon = recon_row.sum()
    kl = 0.0 if kl_row is None else np.asarray(kl_row, np.float64).mean()
    klw = float(np.float32(klw))
    return np.array([recon + klw * kl, recon, kl, klw, *_stats_words(stat, B, Z)]), w, recon_row


def iwae_ref(se_part, logratio, stat, B, K, Z, klw):
    """fp64 (out6, w [K*B], rows3 [3, B]) of mmvae_elbo_finalize_iwae, after oracle.mmvae_oracle.elbo_iwae with
    c = klw / B: lw = -SE - c r, rows3 = (-logmeanexp_k lw, sum_k w SE, sum_k w r), w = softmax_k lw;
    out6 = sum_b bound, sum_b sum_k w SE, mean_b sum_k w r, kl weight, mean(mu), mean(var)."""
    se = np.asarray(se_part, np.float64).sum(0).reshape(K, B)
    r = np.asarray(logratio, np.float64).reshape(K, B)
    klw = float(np.float32(klw))
    lw = -se - (klw / B) * r
    w = _softmax0(lw)
    rows3 = np.stack([-(_logsumexp0(lw) - np.log(K)), (w * se).sum(0), (w * r).sum(0)])
    out6 = np.array([rows3[0].sum(), rows3[1].sum(), rows3[2].mean(), klw, *_stats_words(stat, B, Z)])
    return out6, w.reshape(-1), rows3


def logratio_ref(std, eps, z):
    """std [B, Z], eps / z [K, B, Z] (fp32).  fp64 (r [K, B], sum_j |term_j| [K, B]) with
    term_j = -log s_bj - eps_kbj^2 / 2 + z_kbj^2 / 2."""
    s, e, zz = (np.asarray(a, np.float64) for a in (std, eps, z))
    term = -np.log(s)[None] - 0.5 * e * e + 0.5 * zz * zz
    return term.sum(-1), np.abs(term).sum(-1)


@functools.lru_cache(maxsize=None)
def logratio_inputs(K, B, Z, seed):
    """fp32 (std [B, Z] in [0.05, 3], eps [K, B, Z], z = mu + std * eps rounded as fp32 does)."""
    rng = np.random.default_rng(seed)
    std = np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=(B, Z))).astype(np.float32)
    std = np.clip(std, np.float32(0.05), np.float32(3.0))
    mu = rng.standard_normal((B, Z)).astype(np.float32)
    eps = rng.standard_normal((K, B, Z)).astype(np.float32)
    z = (mu[None] + (std[None] * eps).astype(np.float32)).astype(np.float32)
    return _ro(std, eps, z)


# ---- the two softmax formulas in fp32 (v [K, B] log-weights): what a kernel can reach, and what the defect costs
def _f32_softmax_parts(v):
    v = np.asarray(v, np.float32)
    mx = v.max(0)
    ex = np.exp(v - mx, dtype=np.float32)
    s = np.zeros_like(mx)
    for k in range(v.shape[0]):
        s = (s + ex[k]).astype(np.float32)
    return v, mx, ex, s


def w_lse_form_f32(v):
    """w = expf(v - lse), lse = mx + logf(sum): lse carries the rounding of a number of the size of v."""
    v, mx, ex, s = _f32_softmax_parts(v)
    lse = (mx + np.log(s, dtype=np.float32)).astype(np.float32)
    return np.exp((v - lse).astype(np.float32), dtype=np.float32)


def w_ratio_form_f32(v):
    """w = ex / sum with ex = expf(v - mx): nothing of the size of v is rounded."""
    v, mx, ex, s = _f32_softmax_parts(v)
    return (ex / s).astype(np.float32)


def w_close(w, w_ref, rtol, atol):
    """Elementwise |w - w_ref| <= atol + rtol |w_ref| (torch.testing.assert_close's rule); returns (ok, worst excess
    ratio |w - w_ref| / (atol + rtol |w_ref|))."""
    w, w_ref = np.asarray(w, np.float64).reshape(-1), np.asarray(w_ref, np.float64).reshape(-1)
    ratio = np.abs(w - w_ref) / (atol + rtol * np.abs(w_ref))
    return bool((ratio <= 1.0).all()), float(ratio.max())


def exact_seed(B, K, T):
    return 1000 * B + 10 * K + T
