"""A plain numpy restatement of the FCBlock layer tails, written from the formulas of include/mmvae_hip.h ("FCBlock
layer epilogues", "Fused row tail"), forward and backward: the column tail (mmvae_fc_epilogue_fwd / _bwd), LayerNorm
without affine (mmvae_layernorm_fwd / _bwd) and the row tail (mmvae_fc_rowtail_fwd / _bwd).

Every function takes a `dtype`.  With float64 it is the reference.  With float32 it evaluates the same formulas in the
summation tree the header and the kernel file document, so that a test can measure what fp32 itself loses on an input
(`delta`):
  - slabs are added in slab order, starting from the bias (from zero in backward);
  - column statistics: per chunk of 32 rows a mean and a centred M2 (four groups of eight rows, each summed in row order,
    the four sums as (0 + 1) + (2 + 3)), merged in chunk order with Chan's formula;
  - backward column sums: the same per-chunk sums, added in chunk order;
  - row statistics: two passes, 64 interleaved partial sums per row that are halved pairwise.
Nothing here reads the kernels' results; the ReLU slope of the backward pass is an input (the caller passes the slope
the device took: an activation within rounding of zero may fall on either side in fp32).
"""
import numpy as np

RPC = 32  # rows per chunk of the column statistics and of the [ceil(B / 32)][N] partials


def n_chunks(B):
    return -(-B // RPC)


def _as(x, dtype):
    return None if x is None else np.asarray(x, dtype=dtype)


def slab_sum(slabs, start, dtype):
    """start (a [N] vector or None = zero), then the slabs [S, B, N] in slab order."""
    slabs = _as(slabs, dtype)
    acc = np.zeros(slabs.shape[1:], dtype) if start is None else np.broadcast_to(_as(start, dtype), slabs.shape[1:]).copy()
    for s in range(slabs.shape[0]):
        acc = acc + slabs[s]
    return acc


def chunk_sums(v):
    """[B, N] -> [ceil(B / 32), N]: the column sums of every 32-row chunk (rows beyond B count as zero)."""
    B, N = v.shape
    RC = n_chunks(B)
    padded = np.zeros((RC * RPC, N), v.dtype)
    padded[:B] = v
    groups = padded.reshape(RC, 4, RPC // 4, N)
    s = np.zeros((RC, 4, N), v.dtype)
    for i in range(RPC // 4):
        s = s + groups[:, :, i]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def in_chunk_order(parts):
    """[RC, N] -> [N]: the rows added one after the other."""
    acc = np.zeros(parts.shape[1:], parts.dtype)
    for ch in range(parts.shape[0]):
        acc = acc + parts[ch]
    return acc


def column_stats(z):
    """Batch mean and biased variance of every column of z [B, N]: per-chunk (n, mean, M2), Chan merge in chunk order."""
    dt = z.dtype.type
    B, N = z.shape
    RC = n_chunks(B)
    counts = [min(RPC, B - ch * RPC) for ch in range(RC)]
    cmean = chunk_sums(z) / np.array(counts, z.dtype)[:, None]
    centred = z - np.repeat(cmean, RPC, axis=0)[:B]
    cm2 = chunk_sums(centred * centred)
    n, mean, M2 = dt(0), np.zeros(N, z.dtype), np.zeros(N, z.dtype)
    for ch in range(RC):
        nb = dt(counts[ch])
        delta = cmean[ch] - mean
        nn = n + nb
        mean = mean + delta * (nb / nn)
        M2 = M2 + (cm2[ch] + delta * delta * (n * nb / nn))
        n = nn
    return mean, M2 / dt(B)


def keep_scale(p, dtype):
    dt = np.dtype(dtype).type
    return dt(1) / (dt(1) - dt(np.float32(p)))


def column_fwd(slabs, bias, bn=None, training=True, relu=True, mask=None, p=0.0, dtype=np.float64):
    """z = bias + sum of slabs; [BatchNorm]; [ReLU]; [keep mask].  bn: None or a dict with gamma, beta, running_mean,
    running_var (each an array or None), momentum, eps.  Returns z, y (before the ReLU), a, d and, with BatchNorm in
    training, mean, invstd and the updated running_mean / running_var (None where none were given).
    A batch of one row under training BatchNorm (which torch refuses) has mean = z, variance 0, invstd = 1 / sqrt(eps),
    and moves running_var towards 0."""
    dt = np.dtype(dtype).type
    z = slab_sum(slabs, bias, dtype)
    B = z.shape[0]
    out = dict(z=z, mean=None, invstd=None, running_mean=None, running_var=None)
    y = z
    if bn is not None:
        eps = dt(np.float32(bn["eps"])) if dtype == np.float32 else dt(bn["eps"])
        mom = dt(np.float32(bn["momentum"])) if dtype == np.float32 else dt(bn["momentum"])
        if training:
            mean, var = column_stats(z)
            invstd = dt(1) / np.sqrt(var + eps)
            out.update(mean=mean, invstd=invstd)
            if bn.get("running_mean") is not None:
                out["running_mean"] = (dt(1) - mom) * _as(bn["running_mean"], dtype) + mom * mean
            if bn.get("running_var") is not None:
                unbiased = var * (dt(B) / dt(B - 1)) if B > 1 else var
                out["running_var"] = (dt(1) - mom) * _as(bn["running_var"], dtype) + mom * unbiased
        else:
            mean = _as(bn["running_mean"], dtype)
            invstd = dt(1) / np.sqrt(_as(bn["running_var"], dtype) + eps)
        y = (z - mean) * invstd
        if bn.get("gamma") is not None:
            y = y * _as(bn["gamma"], dtype)
        if bn.get("beta") is not None:
            y = y + _as(bn["beta"], dtype)
    a = np.maximum(y, dt(0)) if relu else y
    d = a
    if mask is not None:
        d = np.where(np.asarray(mask) != 0, a * keep_scale(p, dtype), dt(0))
    out.update(y=y, a=a, d=d)
    return out


def column_dy(din, addend=None, addend_a=None, row_scale=None, mask=None, p=0.0, slope=None, dtype=np.float64):
    """The gradient at the layer's pre-activation output y:
    dd = row_scale * (sum of din slabs + addend); da = (mask ? dd * mask / (1 - p) : dd) + addend_a; dy = da * slope."""
    dt = np.dtype(dtype).type
    g = slab_sum(din, None, dtype)
    if addend is not None:
        g = g + _as(addend, dtype)
    if row_scale is not None:
        g = g * _as(row_scale, dtype)[:, None]
    if mask is not None:
        g = np.where(np.asarray(mask) != 0, g * keep_scale(p, dtype), dt(0))
    if addend_a is not None:
        g = g + _as(addend_a, dtype)
    if slope is not None:
        g = np.where(np.asarray(slope) != 0, g, dt(0))
    return g


def column_bwd(din, fwd=None, gamma=None, addend=None, addend_a=None, row_scale=None, mask=None, p=0.0, slope=None,
               dtype=np.float64):
    """Backward of column_fwd.  fwd: the dict column_fwd returned in the same dtype when the layer has a BatchNorm in
    training (its z, mean, invstd are read), else None.  Returns dy, dz, dbias, dgamma, dbeta and, without BatchNorm,
    `partials`: the [ceil(B / 32)][N] column sums of dz per chunk, whose sum in chunk order is dbias."""
    dt = np.dtype(dtype).type
    dy = column_dy(din, addend, addend_a, row_scale, mask, p, slope, dtype)
    B = dy.shape[0]
    if fwd is None:
        partials = chunk_sums(dy)
        return dict(dy=dy, dz=dy, dbias=in_chunk_order(partials), dgamma=None, dbeta=None, partials=partials)
    mean, invstd = fwd["mean"], fwd["invstd"]
    xhat = (fwd["z"] - mean) * invstd
    S1 = in_chunk_order(chunk_sums(dy))
    S2 = in_chunk_order(chunk_sums(dy * xhat))
    S3 = in_chunk_order(chunk_sums(xhat))
    inv_b = dt(1) / dt(B)
    m1, m2 = S1 * inv_b, S2 * inv_b
    scale = invstd if gamma is None else _as(gamma, dtype) * invstd
    dz = scale * (dy - m1 - xhat * m2)
    # the gradient of a Linear bias ahead of a BatchNorm is zero in exact arithmetic; its closed form: sum_b dz
    return dict(dy=dy, dz=dz, dbias=-scale * m2 * S3, dgamma=S2, dbeta=S1, partials=None)


def row_sums(v):
    """[B, N] -> [B]: 64 interleaved partial sums per row (element j goes to partial j mod 64), halved pairwise."""
    B, N = v.shape
    nv = -(-N // 64)
    padded = np.zeros((B, nv * 64), v.dtype)
    padded[:, :N] = v
    groups = padded.reshape(B, nv, 64)
    s = np.zeros((B, 64), v.dtype)
    for k in range(nv):
        s = s + groups[:, k]
    width = 64
    while width > 1:
        width //= 2
        s = s[:, :width] + s[:, width:2 * width]
    return s[:, 0]


def layernorm_fwd(x, eps, dtype=np.float64):
    """LayerNorm without affine: biased variance, two passes.  Returns y, mean [B], invstd [B]."""
    dt = np.dtype(dtype).type
    x = _as(x, dtype)
    N = x.shape[1]
    eps = dt(np.float32(eps)) if dtype == np.float32 else dt(eps)
    mean = row_sums(x) / dt(N)
    c = x - mean[:, None]
    invstd = dt(1) / np.sqrt(row_sums(c * c) / dt(N) + eps)
    return dict(y=c * invstd[:, None], mean=mean, invstd=invstd)


def layernorm_bwd(g, y, invstd):
    """dx = invstd * (g - mean_row(g) - y * mean_row(g * y)), in the dtype of g."""
    dt = g.dtype.type
    N = g.shape[1]
    m1, m2 = row_sums(g) / dt(N), row_sums(g * y) / dt(N)
    return invstd[:, None] * (g - m1[:, None] - y * m2[:, None])


def rowtail_fwd(slabs, bias, eps, relu=True, mask=None, p=0.0, dtype=np.float64):
    """v = bias + sum of slabs; y = LayerNorm(v); a = relu ? max(y, 0) : y; d = mask ? a * mask / (1 - p) : a."""
    dt = np.dtype(dtype).type
    v = slab_sum(slabs, bias, dtype)
    out = layernorm_fwd(v, eps, dtype)
    a = np.maximum(out["y"], dt(0)) if relu else out["y"]
    d = a if mask is None else np.where(np.asarray(mask) != 0, a * keep_scale(p, dtype), dt(0))
    out.update(v=v, a=a, d=d)
    return out


def rowtail_bwd(din, fwd, addend=None, row_scale=None, mask=None, p=0.0, slope=None, dtype=np.float64):
    """g = row_scale * sum of din slabs; g = (mask ? g * mask / (1 - p) : g) + addend; g = g * slope;
    dz = invstd * (g - mean_row(g) - y * mean_row(g * y)).  Returns dz, partials [ceil(B / 32)][N], dbias."""
    dt = np.dtype(dtype).type
    g = slab_sum(din, None, dtype)
    if row_scale is not None:
        g = g * _as(row_scale, dtype)[:, None]
    if mask is not None:
        g = np.where(np.asarray(mask) != 0, g * keep_scale(p, dtype), dt(0))
    if addend is not None:
        g = g + _as(addend, dtype)
    if slope is not None:
        g = np.where(np.asarray(slope) != 0, g, dt(0))
    dz = layernorm_bwd(g, fwd["y"], fwd["invstd"])
    partials = chunk_sums(dz)
    return dict(dz=dz, partials=partials, dbias=in_chunk_order(partials))


def x3_split(v):
    """Host mirror of the exact three-way bf16 split of fp32 values by truncation (include/mmvae_hip.h, "Pre-split
    operands"): uint16 planes [3, ...] with p0 = the top 16 bits of v, p1 = the top 16 bits of v - p0, p2 = the top 16
    bits of v - p0 - p1 (at most 8 significant bits are left: nothing is lost while that residual is a normal number)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    top = np.uint32(0xFFFF0000)
    u0 = v.view(np.uint32) & top
    r1 = v - u0.view(np.float32)
    u1 = r1.view(np.uint32) & top
    r2 = r1 - u1.view(np.float32)
    u2 = r2.view(np.uint32)
    return np.stack([(u >> np.uint32(16)).astype(np.uint16) for u in (u0, u1, u2)])
