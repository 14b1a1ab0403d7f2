"""UMAP of latent embeddings on the device: what `umap_embeddings` of the reference's runners/umap_predictions.py:25-50
computes with umap-learn, as the three stages of libmmvae_umap.so (include/mmvae_umap.h).

    knn_graph               exact cosine k-nearest neighbours (HIP: fp32 MFMA Gram tiles, running top-k in registers)
    fuzzy_simplicial_set    rho / sigma / memberships per row (HIP), set union G = P + P^T - P o P^T (torch sort/unique)
    find_ab_params          umap-learn's curve fit, on the host
    optimize_layout         deterministic owner-computes SGD epochs (HIP)
    umap_embeddings         the whole call, with the reference function's name and defaults

Device tensors run the HIP kernels, always.  CPU tensors are refused outside `backend.cpu_plumbing()`; inside it every
stage is its statement in fp64 (the tested definition, tests/umap_restatement.py restates it independently).
Deviations from umap-learn are listed in DESIGN.md: exact instead of approximate neighbours, Jacobi instead of in-place
updates, exactly five negatives per firing, Philox negatives, "pca" or "random" start (no spectral init).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import backend
from ._bind import ptr as _ptr, stream as _stream

NEGATIVE_SAMPLE_RATE = 5


@dataclass
class FuzzyGraph:
    """The fuzzy simplicial set as a CSR on the tensors' device, with the per-row quantities it was built from."""
    indptr: torch.Tensor       # [N + 1] int64
    indices: torch.Tensor      # [nnz] int32, sorted within a row
    data: torch.Tensor         # [nnz] fp32 (fp64 on CPU plumbing)
    rho: torch.Tensor          # [N]
    sigma: torch.Tensor        # [N]
    memberships: torch.Tensor  # [N, k]: the directed weights w_ij in front of the set union

    @property
    def n(self) -> int:
        return self.indptr.numel() - 1


# ------------------------------------------------------------------------------------------------------- 1. kNN graph
def knn_graph(X: torch.Tensor, n_neighbors: int = 30, metric: str = "cosine") -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx [N, k] int32, dist [N, k]) of the exact cosine k-nearest-neighbour graph of the rows of X [N, D]: every row
    sorted by (distance, index), rank 0 the point itself at distance 0 (umap-learn's n_neighbors counts the point),
    dist = max(0, 1 - cos), a zero row at distance 1 from every other row.  2 <= k <= 64, k < N, D <= 512."""
    from . import _umap_lib

    if metric != "cosine":
        raise ValueError(f"knn_graph: only metric='cosine' is implemented (got {metric!r})")
    if X.dim() != 2:
        raise ValueError(f"knn_graph: X must be [N, D], got {tuple(X.shape)}")
    N, D = X.shape
    k = int(n_neighbors)
    if not (2 <= k <= _umap_lib.UMAP_MAX_K and k < N and 1 <= D <= _umap_lib.UMAP_MAX_D):
        raise ValueError(f"knn_graph: need 2 <= n_neighbors <= {_umap_lib.UMAP_MAX_K}, n_neighbors < N and D <= "
                         f"{_umap_lib.UMAP_MAX_D} (got N = {N}, D = {D}, n_neighbors = {k})")
    if backend.on_hip(X):
        from . import ops

        if X.dtype != torch.float32:
            raise TypeError(f"knn_graph: expected float32, got {X.dtype}")
        if D > 1 and X.stride(1) != 1:
            X = X.contiguous()
        ldx = X.stride(0) if N > 1 else D
        lib = _umap_lib.load_umap()
        idx = torch.empty((N, k), dtype=torch.int32, device=X.device)
        dist = torch.empty((N, k), dtype=torch.float32, device=X.device)
        nbytes = lib.mmvae_umap_knn_cosine_workspace_bytes(N, D, k)
        ws = ops.workspace(nbytes, X.device, kind="umap_knn")
        _umap_lib.check(lib.mmvae_umap_knn_cosine_f32(N, D, k, _ptr(X), ldx, _ptr(idx), _ptr(dist), _ptr(ws), nbytes,
                                                     _stream()), "mmvae_umap_knn_cosine_f32")
        return idx, dist
    Xd = X.double()
    norm = (Xd * Xd).sum(1).sqrt()
    U = torch.where(norm[:, None] > 0, Xd / torch.where(norm > 0, norm, torch.ones_like(norm))[:, None],
                    torch.zeros_like(Xd))
    full = (1.0 - U @ U.T).clamp_min(0.0)
    keyed = full.clone()
    keyed.fill_diagonal_(-1.0)
    idx = torch.argsort(keyed, dim=1, stable=True)[:, :k]
    dist = torch.gather(full, 1, idx)
    dist[:, 0] = 0.0
    return idx.to(torch.int32), dist


# ------------------------------------------------------------------------------------------------ 2. fuzzy simplicial set
def _smooth_knn_cpu(idx: torch.Tensor, dist: torch.Tensor):
    d64 = dist.double()
    N, k = d64.shape
    target = float(np.log2(k))
    positive = d64 > 0
    first = torch.where(positive, d64, torch.full_like(d64, float("inf"))).min(1).values
    rho = torch.where(torch.isinf(first), torch.zeros_like(first), first)
    d = d64[:, 1:] - rho[:, None]
    lo, mid = torch.zeros(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
    hi = torch.full((N,), float("inf"), dtype=torch.float64)
    done = torch.zeros(N, dtype=torch.bool)
    for _ in range(64):
        psum = torch.where(d > 0, torch.exp(-(d.clamp_min(0.0) / mid[:, None])), torch.ones_like(d)).sum(1)
        done |= (psum - target).abs() < 1e-5
        if bool(done.all()):
            break
        gt = psum > target
        new_mid = torch.where(gt, (lo + mid) / 2.0, torch.where(torch.isinf(hi), mid * 2.0, (mid + hi) / 2.0))
        new_hi, new_lo = torch.where(gt, mid, hi), torch.where(gt, lo, mid)
        lo, hi, mid = torch.where(done, lo, new_lo), torch.where(done, hi, new_hi), torch.where(done, mid, new_mid)
    floor = 1e-3 * torch.where(rho > 0, d64.mean(1), d64.mean().expand(N))
    sigma = torch.maximum(mid, floor)
    dd = d64 - rho[:, None]
    w = torch.where((dd <= 0) | (sigma[:, None] == 0), torch.ones_like(dd), torch.exp(-(dd.clamp_min(0.0) / sigma[:, None])))
    w[idx.long() == torch.arange(N)[:, None]] = 0.0
    return rho, sigma, w


def symmetrise(idx: torch.Tensor, w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(indptr int64, indices int32, data) of G = P + P^T - P o P^T for the directed weights w [N, k] on the edges
    i -> idx[i, j]; explicit zeros dropped, columns sorted.  torch sort/unique on the tensors' device: plumbing."""
    N, k = idx.shape
    dev = idx.device
    rows = torch.arange(N, device=dev, dtype=torch.int64).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    vals = w.reshape(-1)
    live = vals > 0
    rows, cols, vals = rows[live], cols[live], vals[live]
    E = rows.numel()
    uniq, inv = torch.unique(torch.cat([rows * N + cols, cols * N + rows]), sorted=True, return_inverse=True)
    p = torch.zeros(uniq.numel(), dtype=vals.dtype, device=dev)
    pt = torch.zeros_like(p)
    p[inv[:E]] = vals   # (a row of idx holds no column twice: every slot is written once)
    pt[inv[E:]] = vals
    data = p + pt - p * pt
    r = torch.div(uniq, N, rounding_mode="floor")
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0)
    return indptr, (uniq - r * N).to(torch.int32), data


def fuzzy_simplicial_set(idx: torch.Tensor, dist: torch.Tensor) -> FuzzyGraph:
    """umap-learn's fuzzy_simplicial_set (local_connectivity = 1, set_op_mix_ratio = 1) from a kNN graph as knn_graph
    returns it: rho_i the smallest non-zero distance of the row, sigma_i by smooth_knn_dist's bisection, memberships
    w_ij = exp(-max(d_ij - rho_i, 0) / sigma_i) (0 for the point itself), then the set union as a CSR."""
    if idx.shape != dist.shape or idx.dim() != 2:
        raise ValueError(f"fuzzy_simplicial_set: idx {tuple(idx.shape)} vs dist {tuple(dist.shape)}")
    N, k = idx.shape
    if backend.on_hip(dist):
        from . import _umap_lib

        if idx.dtype != torch.int32 or dist.dtype != torch.float32 or idx.device != dist.device:
            raise TypeError("fuzzy_simplicial_set: expected int32 idx and float32 dist on one device")
        idx, dist = idx.contiguous(), dist.contiguous()
        lib = _umap_lib.load_umap()
        mean = dist.mean(dtype=torch.float64).reshape(1)
        rho = torch.empty(N, dtype=torch.float32, device=dist.device)
        sigma = torch.empty_like(rho)
        w = torch.empty_like(dist)
        _umap_lib.check(lib.mmvae_umap_smooth_knn_f32(N, k, _ptr(idx), _ptr(dist), _ptr(mean), _ptr(rho), _ptr(sigma),
                                                     _ptr(w), _stream()), "mmvae_umap_smooth_knn_f32")
    else:
        rho, sigma, w = _smooth_knn_cpu(idx, dist)
    indptr, indices, data = symmetrise(idx, w)
    return FuzzyGraph(indptr, indices, data, rho, sigma, w)


# ------------------------------------------------------------------------------------------------------------ 3. layout
def find_ab_params(spread: float = 1.0, min_dist: float = 0.1) -> Tuple[float, float]:
    """umap-learn's find_ab_params: (a, b) of 1 / (1 + a x^(2b)) fitted by scipy.optimize.curve_fit to 1 below min_dist
    and exp(-(x - min_dist) / spread) above it, on linspace(0, 3 spread, 300)."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def layout_graph(graph: FuzzyGraph, n_epochs: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(indptr int64, indices int32, samples int32) the layout runs on: edges with w < max w / n_epochs dropped, and per
    remaining directed slot e its sample count s_e = max(1, rint(n_epochs w_e / max w)).  Evaluated in fp64."""
    data = graph.data.double()
    N = graph.n
    top = data.max()
    keep = ~(data < top / n_epochs)
    rows = torch.arange(N, device=data.device).repeat_interleave(graph.indptr[1:] - graph.indptr[:-1])[keep]
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=data.device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    samples = torch.round(n_epochs * data[keep] / top).clamp_min(1.0).to(torch.int32)
    return indptr, graph.indices[keep].contiguous(), samples


_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def _philox4x32_10(counter: np.ndarray, stream: int, seed: int) -> np.ndarray:
    """[len(counter), 4] uint32: the device generator's words (counter = c0, c1; stream = c2, c3; seed = the key)."""
    lo, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    counter = np.asarray(counter, dtype=np.uint64)
    c0, c1 = counter & lo, counter >> s32
    c2 = np.full_like(c0, int(stream) & 0xFFFFFFFF)
    c3 = np.full_like(c0, (int(stream) >> 32) & 0xFFFFFFFF)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & lo
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _layout_epoch_cpu(y, rows, indices, samples, n, n_epochs, a, b, gamma, seed):
    N = y.shape[0]
    s = samples.astype(np.int64)
    slots = np.nonzero((n * s) // n_epochs > ((n - 1) * s) // n_epochs)[0]
    i, j = rows[slots], indices[slots]
    total = np.zeros_like(y)

    def add(other, attract):
        diff = y[i] - y[other]
        d2 = (diff * diff).sum(1)
        pos = d2 > 0
        safe = np.where(pos, d2, 1.0)
        if attract:
            coeff = (-2.0 * a * b * safe ** (b - 1.0)) / (a * safe ** b + 1.0)
            g = 2.0 * np.clip(coeff[:, None] * diff, -4.0, 4.0)
            g[~pos] = 0.0
        else:
            coeff = (2.0 * gamma * b) / ((0.001 + safe) * (a * safe ** b + 1.0))
            g = np.clip(coeff[:, None] * diff, -4.0, 4.0)
            g[~pos] = 4.0
            g[other == i] = 0.0
        np.add.at(total, i, g)

    add(j, True)
    e = slots.astype(np.uint64)
    words = np.concatenate([_philox4x32_10(e * np.uint64(2), n, seed),
                            _philox4x32_10(e * np.uint64(2) + np.uint64(1), n, seed)[:, :1]], axis=1).astype(np.uint64)
    neg = ((words * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    for t in range(NEGATIVE_SAMPLE_RATE):
        add(neg[:, t], False)
    return y + (1.0 - (n - 1) / n_epochs) * total


def optimize_layout(y0: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor, samples: torch.Tensor, *,
                    n_epochs: int = 200, a: float, b: float, seed: int = 0, gamma: float = 1.0, first: int = 1,
                    count: Optional[int] = None) -> torch.Tensor:
    """Epochs first .. first + count - 1 (default: through n_epochs) of the layout from state y0 [N, 2 or 3] on the
    pruned graph of `layout_graph`; y0 is left unchanged.  Owner-computes and double-buffered: in epoch n every vertex
    reads the old positions and adds, for each of its edges that fires ((n s_e) div n_epochs steps up), the attraction --
    doubled, for the mirrored edge's "move other" -- and five Philox-drawn repulsions, times alpha_n = 1 - (n - 1) /
    n_epochs.  A pure function of its arguments: no atomics, no races."""
    N, C = y0.shape
    if C not in (2, 3):
        raise ValueError(f"optimize_layout: n_components must be 2 or 3 (got {C})")
    count = n_epochs - first + 1 if count is None else int(count)
    if n_epochs < 1 or first < 1 or count < 0 or first + count - 1 > n_epochs:
        raise ValueError(f"optimize_layout: epochs {first} .. {first + count - 1} are not within 1 .. {n_epochs}")
    if indptr.numel() != N + 1 or indices.numel() != samples.numel():
        raise ValueError("optimize_layout: graph and state disagree")
    if backend.on_hip(y0):
        from . import _umap_lib

        lib = _umap_lib.load_umap()
        ya = y0.to(torch.float32).contiguous().clone()
        yb = torch.empty_like(ya)
        indptr = indptr.to(device=ya.device, dtype=torch.int64).contiguous()
        indices = indices.to(device=ya.device, dtype=torch.int32).contiguous()
        samples = samples.to(device=ya.device, dtype=torch.int32).contiguous()
        _umap_lib.check(lib.mmvae_umap_layout_f32(N, C, _ptr(indptr), _ptr(indices), _ptr(samples), _ptr(ya), _ptr(yb),
                                                 float(a), float(b), float(gamma), int(n_epochs), int(first), count,
                                                 int(seed) & ((1 << 64) - 1), _stream()), "mmvae_umap_layout_f32")
        return yb if count % 2 else ya
    y = y0.double().numpy().copy()
    ptr = indptr.numpy()
    rows = np.repeat(np.arange(N), np.diff(ptr))
    ind, smp = indices.numpy().astype(np.int64), samples.numpy()
    for n in range(first, first + count):
        y = _layout_epoch_cpu(y, rows, ind, smp, n, n_epochs, float(a), float(b), float(gamma), int(seed))
    return torch.from_numpy(y)


def initial_layout(X: torch.Tensor, n_components: int = 2, init: str = "pca", seed: int = 0) -> torch.Tensor:
    """The start of the layout, [N, n_components]: "pca" -- the first principal components (eigenvectors of the centred
    D x D scatter matrix, each signed so that its largest loading is positive) scaled so that the largest coordinate is
    10; "random" -- uniform in +-10, element m = word m % 4 of philox4x32_10(m // 4, stream 0, seed)."""
    N = X.shape[0]
    on_hip = backend.on_hip(X)
    if init == "random":
        if on_hip:
            from . import _umap_lib

            y = torch.empty((N, n_components), dtype=torch.float32, device=X.device)
            _umap_lib.check(_umap_lib.load_umap().mmvae_umap_random_init_f32(y.numel(), _ptr(y), int(seed) & ((1 << 64) - 1),
                                                                           _stream()), "mmvae_umap_random_init_f32")
            return y
        n = N * n_components
        words = _philox4x32_10(np.arange((n + 3) // 4, dtype=np.uint64), 0, seed).reshape(-1)[:n]
        u = ((words >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
        return torch.from_numpy((20.0 * u.astype(np.float64) - 10.0).reshape(N, n_components))
    if init != "pca":
        raise ValueError(f"initial_layout: init must be 'pca' or 'random' (got {init!r}; there is no spectral init)")
    Xc = X.double()
    Xc = Xc - Xc.mean(0)
    _, vec = np.linalg.eigh((Xc.T @ Xc).cpu().numpy())  # D x D on the host: D <= 512
    V = vec[:, ::-1][:, :n_components]
    V = V * np.sign(V[np.abs(V).argmax(0), np.arange(n_components)])
    proj = Xc @ torch.from_numpy(np.ascontiguousarray(V)).to(Xc.device)
    y = 10.0 * proj / proj.abs().max()
    return y.float() if on_hip else y


def umap_embeddings(X: torch.Tensor, n_neighbors: int = 30, min_dist: float = 0.3, n_components: int = 2,
                    metric: str = "cosine", low_memory: bool = False, n_jobs: int = 40, n_epochs: int = 200,
                    init: str = "pca", seed: int = 0, spread: float = 1.0, **ignored) -> torch.Tensor:
    """`umap_embeddings` of the reference (runners/umap_predictions.py:25-50), same name and defaults: the UMAP of the
    rows of X [N, D] as a tensor [N, n_components] on X's device.  `low_memory`, `n_jobs` and any further keyword are
    accepted and ignored (they steer umap-learn's CPU implementation).  Deterministic in (X, arguments, seed)."""
    if metric != "cosine":
        raise ValueError(f"umap_embeddings: only metric='cosine' is implemented (got {metric!r})")
    if n_components not in (2, 3):
        raise ValueError(f"umap_embeddings: n_components must be 2 or 3 (got {n_components})")
    idx, dist = knn_graph(X, n_neighbors, metric)
    graph = fuzzy_simplicial_set(idx, dist)
    a, b = find_ab_params(spread, min_dist)
    y0 = initial_layout(X, n_components, init, seed)
    indptr, indices, samples = layout_graph(graph, int(n_epochs))
    return optimize_layout(y0, indptr, indices, samples, n_epochs=int(n_epochs), a=a, b=b, seed=seed)
