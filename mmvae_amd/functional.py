"""torch.autograd.Function wrappers: the module-level (flexible) execution path of the mirror.

Every tensor-sized operation below -- forward and backward -- is a call into libmmvae_hip.so through mmvae_amd.ops.
Autograd only sequences them.  0-dim loss bookkeeping (adding two scalar losses, dividing by the batch size) is left
to torch scalar ops; the graph-captured step engine (mmvae_amd.engine) does even that inside kernels.

Reference call sites these replace are cited per class (paths relative to /root/reference/src/cmmvae/).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


class FCLayerFn(torch.autograd.Function):
    """One FCBlock layer: Linear -> [BatchNorm1d] -> [ReLU] -> [Dropout]  (modules/base/components.py:275-290).

    Returns (d, a): d = layer output (post dropout), a = post-activation / pre-dropout tensor, which is what
    FCBlock.forward collects as a hidden representation (components.py:312-313).  a is d when there is no dropout.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, bn_state, training, relu, keep_mask, dropout_p):
        x2 = x if x.is_contiguous() else x.contiguous()
        B, N = x2.shape[0], weight.shape[0]
        has_bn = bn_state is not None
        ctx.has_bn, ctx.relu, ctx.p = has_bn, relu, dropout_p
        ctx.training = training
        use_mask = keep_mask is not None and training and dropout_p > 0
        _, splitk = ops.gemm_plan(ops.GEMM_NT, B, N, x2.shape[1])
        if not has_bn and not use_mask and splitk == 1:
            d = ops.gemm(ops.GEMM_NT, x2, weight, bias=bias, relu=relu, splitk=1)  # bias/ReLU in the GEMM epilogue
            a = d
            z = mean = invstd = None
        else:
            slabs = ops.gemm_slabs(ops.GEMM_NT, x2, weight, splitk=splitk)
            bn = None
            if has_bn:
                bn = dict(gamma=gamma, beta=beta, running_mean=bn_state["running_mean"],
                          running_var=bn_state["running_var"],
                          num_batches_tracked=bn_state.get("num_batches_tracked"),
                          momentum=bn_state["momentum"], eps=bn_state["eps"])
            f = ops.fc_epilogue_fwd(slabs, bias, bn=bn, training=training, relu=relu,
                                    keep_mask=keep_mask if use_mask else None, dropout_p=dropout_p)
            d, a, z, mean, invstd = f["d"], f["a"], f["z"], f["mean"], f["invstd"]
        ctx.use_mask = use_mask
        ctx.save_for_backward(x2, weight, gamma, a, z, mean, invstd, keep_mask if use_mask else None)
        if a is d:
            return d  # no dropout: the hidden representation IS the layer output
        return d, a

    @staticmethod
    def backward(ctx, gd, ga=None):
        x, weight, gamma, a, z, mean, invstd, mask = ctx.saved_tensors
        if ctx.has_bn and not ctx.training:
            raise RuntimeError("backward through eval-mode BatchNorm is not part of the training step")
        gd = gd.contiguous() if gd is not None else None
        ga = ga.contiguous() if ga is not None else None
        if gd is None and ga is None:
            return (None,) * 10
        # gd: gradient on the layer output d (through the keep mask); ga: gradient on the pre-dropout activation, which
        # bypasses the mask (addend_a of the layer-tail kernel)
        if gd is None:
            gd, ga, mask_arg, p = ga, None, None, 0.0
        else:
            mask_arg, p = (mask, ctx.p) if ctx.use_mask else (None, 0.0)
        dz, dbias, dgamma, dbeta = ops.fc_epilogue_bwd(
            gd, addend_a=ga, keep_mask=mask_arg, dropout_p=p, relu=ctx.relu, a=a if ctx.relu else None, z=z,
            gamma=gamma, mean=mean, invstd=invstd, has_bn=ctx.has_bn)
        dw = ops.gemm(ops.GEMM_TN, dz, x) if ctx.needs_input_grad[1] else None
        dx = ops.gemm(ops.GEMM_NN, dz, weight) if ctx.needs_input_grad[0] else None
        return dx, dw, dbias if ctx.needs_input_grad[2] else None, dgamma, dbeta, None, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm(elementwise_affine=False) (components.py:281)."""

    @staticmethod
    def forward(ctx, x, eps):
        y, invstd = ops.layernorm_fwd(x.contiguous(), eps)
        ctx.save_for_backward(y, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, invstd = ctx.saved_tensors
        return ops.layernorm_bwd(gy.contiguous(), y, invstd), None


class LayerTailFn(torch.autograd.Function):
    """[ReLU] -> [Dropout] as a pass of its own (the tail of an FCBlock layer whose LayerNorm separates it from the
    Linear's column kernel, components.py:281-288).  Returns (d, a): output and pre-dropout activation."""

    @staticmethod
    def forward(ctx, x, relu, keep_mask, dropout_p):
        use_mask = keep_mask is not None and dropout_p > 0
        f = ops.fc_epilogue_fwd(x.contiguous(), None, relu=relu, keep_mask=keep_mask if use_mask else None,
                                dropout_p=dropout_p if use_mask else 0.0)
        d, a = f["d"], f["a"]
        ctx.relu, ctx.p, ctx.use_mask = relu, dropout_p, use_mask
        ctx.save_for_backward(a if relu else None, keep_mask if use_mask else None)
        if a is d:
            return d
        return d, a

    @staticmethod
    def backward(ctx, gd, ga=None):
        a, mask = ctx.saved_tensors
        gd = gd.contiguous() if gd is not None else None
        ga = ga.contiguous() if ga is not None else None
        if gd is None and ga is None:
            return None, None, None, None
        if gd is None:
            gd, ga, mask_arg, p = ga, None, None, 0.0
        else:
            mask_arg, p = (mask, ctx.p) if ctx.use_mask else (None, 0.0)
        dx, _, _, _ = ops.fc_epilogue_bwd(gd, addend_a=ga, keep_mask=mask_arg, dropout_p=p, relu=ctx.relu,
                                          a=a if ctx.relu else None, want_dbias=False)
        return dx, None, None, None


def layer_tail(x, *, relu: bool, keep_mask=None, dropout_p: float = 0.0):
    out = LayerTailFn.apply(x, relu, keep_mask, dropout_p)
    return out if isinstance(out, tuple) else (out, out)


class CondLinearFn(torch.autograd.Function):
    """Per-cell conditional Linear, y[b] = W[c_b] x[b] + bias[c_b] (ConditionalLayer.forward, components.py:365-413,
    for single-Linear condition blocks), on the grouped HIP kernels.  The thousands of condition blocks are not autograd
    inputs: they are addressed through their offsets in the optimiser's arena (`bank`), and backward writes the
    gradients of the conditions PRESENT in the batch straight into the gradient arena and tells the optimiser which
    parameters took part (the others keep "no gradient", like under torch autograd)."""

    @staticmethod
    def forward(ctx, x, bank, tables, present_params):
        x2 = x if x.is_contiguous() else x.contiguous()
        a = bank["opt"].arena
        y = ops.cond_linear_fwd(x2, a.data, bank["w_off"], bank["b_off"], tables["cond"], bank["n_out"], rows=tables["rows"])
        ctx.save_for_backward(x2)
        ctx.bank, ctx.tables, ctx.present_params = bank, tables, present_params
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        bank = ctx.bank
        opt = bank["opt"]
        a = opt.arena
        gy = gy if gy.is_contiguous() else gy.contiguous()
        dx = ops.cond_linear_bwd(gy, x, a.data, a.grad, bank["w_off"], bank["b_off"], ctx.tables)
        opt.note_direct_grads(ctx.present_params)
        return dx, None, None, None


class ReparamKLFn(torch.autograd.Function):
    """Encoder tail (components.py:795-801) fused with the Gaussian KL of BaseVAE.elbo (modules/vae.py:136-137).

    (mu, a_raw, eps) -> z = mu + sqrt(exp(a_raw) + var_eps) * eps, std, kl_sum = sum_b sum_j KL_bj.
    eps: [B,Z] or [K,B,Z] (K-sample extension).  Also caches, non-differentiably, sum(mu) and sum(var) for the
    Mean / Variance log lines (models/cmmvae_model.py:170-171)."""

    @staticmethod
    def forward(ctx, mu, a_raw, eps, var_eps):
        mu, a_raw, eps = mu.contiguous(), a_raw.contiguous(), eps.contiguous()
        std, z, kl_row, stat = ops.reparam_kl_fwd(mu, a_raw, eps, var_eps)
        kl_sum = ops.sum_f32(kl_row).reshape(())
        ctx.var_eps = var_eps
        ctx.save_for_backward(mu, std, eps)
        ctx.mark_non_differentiable(stat)
        return z, std, kl_sum, stat

    @staticmethod
    def backward(ctx, gz, gstd, gkl, _gstat):
        mu, std, eps = ctx.saved_tensors
        gz = gz.contiguous() if gz is not None else None
        gstd = gstd.contiguous() if gstd is not None else None
        if gkl is not None:
            dmu, da = ops.reparam_kl_bwd(mu, std, eps, gz, dstd_extra=gstd, kl_scale_dev=gkl.contiguous(),
                                         var_eps=ctx.var_eps)
        else:
            dmu, da = ops.reparam_kl_bwd(mu, std, eps, gz, dstd_extra=gstd, kl_scale=0.0, var_eps=ctx.var_eps)
        return dmu, da, None, None


class MseSumFn(torch.autograd.Function):
    """F.mse_loss(xhat, x, reduction="sum") (modules/vae.py:143): per-cell squared error rows + their sum."""

    @staticmethod
    def forward(ctx, xhat, x):
        se_row, _ = ops.mse_sum_fwd_bwd(xhat, x, want_grad=False)
        ctx.save_for_backward(xhat, x)
        return ops.sum_f32(se_row).reshape(())

    @staticmethod
    def backward(ctx, g):
        xhat, x = ctx.saved_tensors
        _, dx = ops.mse_sum_fwd_bwd(xhat, x, want_grad=True, gscale_dev=g.contiguous())
        return dx, None


class KSampleReconFn(torch.autograd.Function):
    """K-sample reconstruction term (extension): sum_b -logmeanexp_k(-||x_b - xhat_bk||^2).
    xhat: [K*B, G] (sample-major), x: [B, G].  Reduces to MseSumFn at K = 1."""

    @staticmethod
    def forward(ctx, xhat, x, K):
        B = x.shape[0]
        xr = x.repeat(K, 1) if K > 1 else x  # plumbing copy; the engine path compares against x[r % B] in-kernel
        se_row, _ = ops.mse_sum_fwd_bwd(xhat, xr, want_grad=False)
        out, w = ops.elbo_finalize(se_row.reshape(1, -1), None, None, B=B, K=K, want_w=True)
        ctx.save_for_backward(xhat, xr, w)
        return out[1].reshape(())

    @staticmethod
    def backward(ctx, g):
        xhat, xr, w = ctx.saved_tensors
        _, d = ops.mse_sum_fwd_bwd(xhat, xr, want_grad=True, gscale_dev=g.contiguous())
        return ops.scale_rows(d, w), None, None


class CrossEntropySumFn(torch.autograd.Function):
    """nn.CrossEntropyLoss(reduction="sum") on adversarial head logits (models/cmmvae_model.py:54,85)."""

    @staticmethod
    def forward(ctx, logits, labels):
        rows, _ = ops.cross_entropy_sum(logits, labels, want_grad=False)
        ctx.save_for_backward(logits, labels)
        return ops.sum_f32(rows).reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, labels = ctx.saved_tensors
        _, dl = ops.cross_entropy_sum(logits, labels, want_grad=True, gscale_dev=g.contiguous())
        return dl, None


class GradientReversalFunction(torch.autograd.Function):
    """Gradient reversal layer (components.py:879-899): identity forward, -alpha * grad backward."""

    @staticmethod
    def forward(ctx, x, alpha):
        ctx.alpha = alpha
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad_output):
        if grad_output.is_cuda:
            g = grad_output.contiguous()
            return ops.axpby(-float(ctx.alpha), g, 0.0, torch.empty_like(g)), None
        return grad_output.neg() * ctx.alpha, None  # CPU plumbing


def fc_layer(x, weight, bias, *, gamma=None, beta=None, bn_state: Optional[dict] = None, training=True, relu=False,
             keep_mask=None, dropout_p=0.0):
    """Returns (d, a): layer output and post-activation / pre-dropout tensor (the same object without dropout)."""
    out = FCLayerFn.apply(x, weight, bias, gamma, beta, bn_state, training, relu, keep_mask, dropout_p)
    return out if isinstance(out, tuple) else (out, out)


def col_pearson(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Per-gene Pearson correlation r [G] of two [cells, genes] matrices, NaN where a column of either is constant --
    the statistic of runners/cross_generation.py:87-152 and runners/correlations.py:69-115.  Device tensors: one
    read-once HIP launch (ops.col_pearson).  CPU tensors only under backend.cpu_plumbing(): the centred two-pass
    statement in fp64 (host-logic tests)."""
    from . import backend

    if backend.on_hip(a):
        return ops.col_pearson(a, b)
    da, db = a.double() - a.double().mean(0), b.double() - b.double().mean(0)
    r = (da * db).sum(0) / torch.sqrt((da * da).sum(0) * (db * db).sum(0))
    constant = (a == a[0]).all(0) | (b == b[0]).all(0)
    return torch.where(constant, torch.full_like(r, float("nan")), r.clamp(-1.0, 1.0)).float()


def row_corrcoef(a: torch.Tensor, b: Optional[torch.Tensor] = None, *, want_matrix: bool = True):
    """(corr, stats) of the ROWS of the stacked [n_a + n_b, genes] matrix (a ; b) -- `np.corrcoef` of a cis generation
    stacked on a cross generation and the block means calc_correlations (runners/run_correlations.py:18-60) reports.
    corr [R, R]: clamped to [-1, 1], NaN in the row and column of every constant row (numpy's 0 / 0), 1 on the rest of
    the diagonal.  stats float64[8]: the nan_to_num means of corr[:n_a, :n_a] (cis), corr[n_a:, n_a:] (cross) and
    corr[:n_a, n_a:] (comb), 2 comb / (cis + cross), the constant-row counts of a and of b, 0, 0; NaN for the three
    statistics that need b when there is none.  Device tensors: the HIP kernels of libmmvae_stats.so
    (ops.row_corrcoef; corr fp32, nothing is stacked).  CPU tensors only under backend.cpu_plumbing(): the centred
    statement in fp64, corr returned as fp64 (host-logic tests).  want_matrix=False: corr is None (on the device it is
    then never stored)."""
    from . import backend

    if backend.on_hip(a):
        return ops.row_corrcoef(a, b, want_matrix=want_matrix)
    n_a = a.shape[0]
    x = a.double() if b is None else torch.cat([a.double(), b.double()], 0)
    n_b = x.shape[0] - n_a
    d = x - x.mean(1, keepdim=True)
    cov = d @ d.T
    var = cov.diagonal()
    corr = (cov / torch.sqrt(var[:, None] * var[None, :])).clamp(-1.0, 1.0)
    corr.fill_diagonal_(1.0)
    constant = (x == x[:, :1]).all(1)
    corr[constant, :] = float("nan")
    corr[:, constant] = float("nan")
    z = torch.nan_to_num(corr, nan=0.0)
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    cis = z[:n_a, :n_a].mean()
    cross = z[n_a:, n_a:].mean() if n_b else nan
    comb = z[:n_a, n_a:].mean() if n_b else nan
    stats = torch.zeros(8, dtype=torch.float64)
    stats[0], stats[1], stats[2], stats[3] = cis, cross, comb, 2.0 * comb / (cis + cross)
    stats[4], stats[5] = constant[:n_a].sum(), constant[n_a:].sum()
    return (corr if want_matrix else None), stats


def meta_disc_tail(pre1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, W3: torch.Tensor, b3: torch.Tensor,
                   y: Optional[torch.Tensor] = None, *, train: bool = False):
    """A meta-discriminator (runners/meta_discriminators.py:16-55, :131-163) behind its first layer, with its loss and
    its backward: (p, out, dpre1, grads).

        h1 = sigmoid(pre1)    h2 = sigmoid(h1 W2^T + b2)    s = h2 . W3 + b3    p = sigmoid(s)          p: [B]
        loss_row = y min(softplus(-s), 100) + (1 - y) min(softplus(s), 100)   (torch's -log clamped at -100)
        out = [mean of loss_row, fraction of rows with (p > 0.5) == (y > 0.5)]             (None without y)

    train=True: the gradients of that MEAN, ds = (p - y) / B chained back: dpre1 [B, H1] and grads = (db1, dW2, db2,
    dW3, db3) in the shapes of the parameters; both None otherwise.  This is F.binary_cross_entropy(reduction="mean")
    under autograd wherever p (1 - p) >= 1e-12; past that torch clamps the gradient away, this one stays p - y (formed
    as (1 - y) sigmoid(s) - y sigmoid(-s); sigmoid' as sigmoid(x) sigmoid(-x), so that no tail cancels).
    Device tensors: the two HIP launches of libmmvae_disc.so (ops.disc_tail, fp32).  CPU tensors only under
    backend.cpu_plumbing(): this statement in fp64, returned as fp64 -- the tested definition."""
    from . import backend

    if backend.on_hip(pre1):
        return ops.disc_tail(pre1, W2, b2, W3, b3, y, train=train)
    sig, sp = torch.sigmoid, torch.nn.functional.softplus
    x, w2, w3 = pre1.double(), W2.double(), W3.double().reshape(-1)
    B = x.shape[0]
    h1 = sig(x)
    a2 = h1 @ w2.T + b2.double()
    h2 = sig(a2)
    s = h2 @ w3 + b3.double().reshape(())
    p = sig(s)
    if y is None:
        if train:
            raise ValueError("meta_disc_tail: train=True needs y")
        return p, None, None, None
    yd = y.double().reshape(-1)
    loss_row = yd * sp(-s).clamp(max=100.0) + (1.0 - yd) * sp(s).clamp(max=100.0)
    out = torch.stack([loss_row.mean(), ((p > 0.5) == (yd > 0.5)).double().mean()])
    if not train:
        return p, out, None, None
    ds = ((1.0 - yd) * p - yd * sig(-s)) / B
    da2 = ds[:, None] * w3[None, :] * h2 * sig(-a2)
    dpre1 = (da2 @ w2) * h1 * sig(-x)
    grads = (dpre1.sum(0), da2.T @ h1, da2.sum(0), (h2.T @ ds).reshape(W3.shape), ds.sum().reshape(1))
    return p, out, dpre1, grads
