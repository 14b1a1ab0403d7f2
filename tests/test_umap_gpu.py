"""libmmvae_umap.so on the GPU against the fp64 restatement (tests/umap_restatement.py).

kNN bound (derived, not measured): a dot product of two fp32 unit rows is one D-long fmaf chain, |error| <= D 2^-24
sum |u_i u_j| <= D 2^-24; the unit rows carry 2 roundings each (reciprocal norm, product), which moves the dot product by
at most 4 2^-24 more per unit of sum |u_i u_j|, and 1 - dot and the store add 2^-24 each: atol = (2 D + 8) 2^-24 with
room to spare.  Indices are compared wherever the fp64 gaps to both neighbouring ranks exceed 2 atol -- there fp32
cannot reorder them.

Fuzzy set: the kernel stops its fp64 bisection at 1e-5 and rounds sigma to fp32 (<= 63 * 0.37 * 2^-24 = 1.4e-6 in the
sum): 2e-5.  Layout: one epoch at a time from the restatement's own states, held to 4 delta where delta is what the
restatement itself loses when it is evaluated in fp32 from the same state with the same negatives.  Each test prints
the figures it measured."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import umap_restatement as R

pytestmark = pytest.mark.gpu

# (N, D, k, leading dimension)
#   (300, 128, 30)     five row blocks of 64 and 5 column tiles, the last of each ragged
#   (257, 50, 15) ld 56: rows that are no 16-byte groups, D off every vector width and off the 64-column chunk
#   (16, 8, 15)        every other point is a neighbour; one partial tile
#   (5000, 128, 30)    79 column tiles, 79 workgroups
#   (300, 128, 64/2)   the limits on k
#   (200, 300, 10)     D > 256: the 512-column variant, 8 staged chunks per tile;  (150, 200, 10): the 256-column one
KNN_CASES = [(300, 128, 30, 128), (257, 50, 15, 56), (16, 8, 15, 8), (5000, 128, 30, 128), (300, 128, 64, 128),
             (300, 128, 2, 128), (200, 300, 10, 300), (150, 200, 10, 201)]
KNN_IDS = [f"{c[0]}x{c[1]}k{c[2]}" for c in KNN_CASES]


def knn_atol(D):
    return (2 * D + 8) * 2.0 ** -24


def on_device(X, ld):
    """X on the GPU as a view with leading dimension ld."""
    buf = torch.full((X.shape[0], ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :X.shape[1]] = torch.from_numpy(X).cuda()
    return buf[:, :X.shape[1]]


def check_knn(X, k, idx, dist, what):
    """Every property of the issue for one kNN result; returns the share of entries whose index could not be compared."""
    N, D = X.shape
    atol = knn_atol(D)
    oidx, odist, full = R.cosine_knn(X, min(k + 1, N))
    assert idx.shape == (N, k) and dist.shape == (N, k) and idx.dtype == np.int32 and dist.dtype == np.float32
    assert np.array_equal(idx[:, 0], np.arange(N)) and (dist[:, 0] == 0).all()
    assert (idx >= 0).all() and (idx < N).all()
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a neighbour twice in a row"
    dd, di = np.diff(dist.astype(np.float64), axis=1), np.diff(idx.astype(np.int64), axis=1)
    assert ((dd[:, 1:] > 0) | ((dd[:, 1:] == 0) & (di[:, 1:] > 0))).all(), "rows are not sorted by (distance, index)"
    assert (dd[:, 0] >= 0).all()
    rank_err = np.abs(dist - odist[:, :k]).max()
    np.fill_diagonal(full, 0.0)
    own_err = np.abs(np.take_along_axis(full, idx.astype(np.int64), axis=1) - dist).max()
    gaps = np.diff(odist, axis=1) > 2 * atol  # gaps[:, r]: between ranks r and r + 1
    if gaps.shape[1] < k:  # k + 1 > N: nothing lies behind the last rank
        gaps = np.concatenate([gaps, np.ones((N, 1), dtype=bool)], axis=1)
    firm = np.ones((N, k), dtype=bool)
    firm[:, 1:] &= gaps[:, 1:k]
    firm[:, 2:] &= gaps[:, 1:k - 1]
    left_out = 1.0 - firm.mean()
    print(f"{what}: rank-wise error {rank_err:.3g}, own-index error {own_err:.3g} (atol {atol:.3g}), "
          f"{100 * left_out:.2f} % of indices not comparable")
    assert rank_err <= atol and own_err <= atol
    assert np.array_equal(idx[firm], oidx[:, :k][firm])
    assert left_out <= 0.05
    return left_out


@pytest.mark.parametrize("N, D, k, ld", KNN_CASES, ids=KNN_IDS)
def test_knn_against_fp64_brute_force(N, D, k, ld):
    from mmvae_amd import umap as U

    X = np.random.default_rng(0).standard_normal((N, D)).astype(np.float32)
    idx, dist = U.knn_graph(on_device(X, ld), k)
    torch.cuda.synchronize()
    check_knn(X, k, idx.cpu().numpy(), dist.cpu().numpy(), f"kNN {N}x{D} k={k}")


def test_knn_refuses_k_of_n_or_more():
    from mmvae_amd import _umap_lib
    from mmvae_amd import umap as U

    x = torch.randn(16, 8, device="cuda")
    lib = _umap_lib.load_umap()
    idx = torch.full((16, 16), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((16, 16), -7.0, device="cuda")
    ws = torch.empty(1 << 16, device="cuda")
    for k in (16, 17):
        assert lib.mmvae_umap_knn_cosine_workspace_bytes(16, 8, k) == 0
        rc = lib.mmvae_umap_knn_cosine_f32(16, 8, k, x.data_ptr(), 8, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
        assert rc == _umap_lib.ERR_ARG
        with pytest.raises(ValueError, match="n_neighbors"):
            U.knn_graph(x, k)
    torch.cuda.synchronize()
    assert (idx == -7).all() and (dist == -7.0).all()  # nothing was launched


def _duplicates_and_zero_row():
    X = np.random.default_rng(4).standard_normal((200, 40)).astype(np.float32)
    X[11] = X[10]
    X[12] = 3.0 * X[10]  # the same direction
    X[50] = 0.0
    X[100:120] = X[100]  # a row whose every neighbour is a duplicate (k = 15)
    return X


def test_knn_duplicates_and_zero_row():
    from mmvae_amd import umap as U

    X = _duplicates_and_zero_row()
    k, atol = 15, knn_atol(40)
    idx, dist = U.knn_graph(torch.from_numpy(X).cuda(), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    _, odist, _ = R.cosine_knn(X, k)
    print("duplicates: distances of row 10", dist[10, :4], "of row 100", dist[100, :4])
    assert np.abs(dist - odist).max() <= atol
    assert np.array_equal(idx[:, 0], np.arange(200)) and (dist[:, 0] == 0).all()
    assert (dist[10, 1:3] <= atol).all() and set(idx[10, 1:3]) == {11, 12}
    assert (dist[100:120, :] <= atol).all()
    assert (dist[50, 1:] == 1.0).all() and np.array_equal(idx[50, 1:], np.arange(k - 1))  # ties in index order
    others = np.delete(np.arange(200), 50)
    assert not (idx[others] == 50).any() or (dist[others][idx[others] == 50] == 1.0).all()


@pytest.fixture(scope="module")
def fuzzy_case():
    from mmvae_amd import umap as U

    X = np.random.default_rng(0).standard_normal((300, 128)).astype(np.float32)
    idx, dist = U.knn_graph(torch.from_numpy(X).cuda(), 30)
    g = U.fuzzy_simplicial_set(idx, dist)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), g


def test_fuzzy_rho_and_sigma(fuzzy_case):
    idx, dist, g = fuzzy_case
    rho, sigma = g.rho.cpu().numpy(), g.sigma.cpu().numpy()
    assert rho.dtype == np.float32 and sigma.dtype == np.float32
    first = np.array([row[row > 0][0] for row in dist], dtype=np.float32)
    assert np.array_equal(rho.view(np.uint32), first.view(np.uint32))
    err = np.abs(R.smooth_sum(dist, rho, sigma) - np.log2(30))
    rsigma, _ = R.smooth_knn_dist(dist)
    print(f"fuzzy set: |sum - log2 k| max {err.max():.3g}; sigma against the restatement's own bisection "
          f"{np.abs(sigma - rsigma).max():.3g}")
    assert err.max() <= 2e-5
    assert (sigma > 1e-3 * dist.mean(1)).all()  # none of these rows is at its floor


def test_fuzzy_memberships_and_csr(fuzzy_case):
    idx, dist, g = fuzzy_case
    rho, sigma = g.rho.cpu().numpy(), g.sigma.cpu().numpy()
    w = g.memberships.cpu().numpy()
    want_w = R.membership_strengths(idx, dist, rho, sigma)
    assert (w[:, 0] == 0).all() and np.abs(w - want_w).max() <= 1e-6
    assert np.array_equal(w == 0, want_w == 0)
    ptr, ind, data = R.symmetrise(idx, want_w)
    assert g.indptr.dtype == torch.int64 and g.indices.dtype == torch.int32 and g.data.dtype == torch.float32
    assert np.array_equal(g.indptr.cpu().numpy(), ptr) and np.array_equal(g.indices.cpu().numpy(), ind)
    err = np.abs(g.data.cpu().numpy() - data).max()
    print(f"fuzzy set: memberships {np.abs(w - want_w).max():.3g}, symmetrised values {err:.3g} from the restatement")
    assert err <= 1e-6
    # symmetric, with sorted columns
    dense = np.zeros((300, 300))
    rows = np.repeat(np.arange(300), np.diff(ptr))
    dense[rows, g.indices.cpu().numpy()] = g.data.cpu().numpy()
    assert np.array_equal(dense, dense.T)


def test_fuzzy_row_of_duplicates_gets_the_floor():
    from mmvae_amd import umap as U

    X = _duplicates_and_zero_row()
    idx, dist = U.knn_graph(torch.from_numpy(X).cuda(), 15)
    g = U.fuzzy_simplicial_set(idx, dist)
    d = dist.cpu().numpy().astype(np.float64)
    rho, sigma = g.rho.cpu().numpy(), g.sigma.cpu().numpy()
    for i in range(100, 120):
        floor = 1e-3 * (d[i].mean() if rho[i] > 0 else d.mean())
        assert abs(sigma[i] - floor) <= 1e-6 * floor + 1e-45, (i, sigma[i], floor)
    nz = np.array([row[row > 0][0] if (row > 0).any() else 0.0 for row in dist.cpu().numpy()], dtype=np.float32)
    assert np.array_equal(rho, nz)
    assert sigma[50] > 0 and np.isfinite(sigma).all() and np.isfinite(g.data.cpu().numpy()).all()
    assert (g.memberships[50, 1:] == 1.0).all()  # the zero row: every neighbour at rho = 1


# ---------------------------------------------------------------------------------------------------------- the layout
K12, EPOCHS, SEED = 15, 200, 1
KEPT = (1, 50, 150)


@pytest.fixture(scope="module")
def cluster_run():
    """The 12-cluster set, its restated graph, and one restated 200-epoch run (2-D, pca start) with the states in front
    of epochs 1, 50 and 150: computed once, never modified."""
    X, labels = R.clusters()
    idx, dist, _ = R.cosine_knn(X, K12)
    ptr, ind, data = R.fuzzy_simplicial_set(idx, dist)
    pptr, pind, psmp = R.prune_and_samples(ptr, ind, data, EPOCHS)
    a, b = R.find_ab_params(1.0, 0.3)
    final, kept = R.optimize_layout(R.pca_init(X, 2), pptr, pind, psmp, EPOCHS, a, b, SEED, keep=KEPT)
    return dict(X=X, labels=labels, graph=(pptr, pind, psmp), a=a, b=b, final=final, kept=kept)


@pytest.mark.parametrize("n", KEPT)
def test_layout_one_epoch_from_a_restated_state(cluster_run, n):
    from mmvae_amd import umap as U

    c = cluster_run
    pptr, pind, psmp = c["graph"]
    state = c["kept"][n].astype(np.float32)
    want = R.layout_epoch(state.astype(np.float64), pptr, pind, psmp, n, EPOCHS, c["a"], c["b"], SEED)
    in_fp32 = R.layout_epoch(state, pptr, pind, psmp, n, EPOCHS, c["a"], c["b"], SEED, dtype=np.float32)
    delta = np.abs(in_fp32.astype(np.float64) - want).max()
    y0 = torch.from_numpy(state).cuda()
    got = U.optimize_layout(y0, torch.from_numpy(pptr).cuda(), torch.from_numpy(pind).cuda(),
                            torch.from_numpy(psmp).cuda(), n_epochs=EPOCHS, a=c["a"], b=c["b"], seed=SEED, first=n, count=1)
    assert torch.equal(y0.cpu(), torch.from_numpy(state))  # the input state is left alone
    dev = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    moved = np.abs(want - state).max()
    print(f"layout epoch {n}: device {dev:.3g} from the fp64 restatement, the restatement in fp32 {delta:.3g} "
          f"(largest move {moved:.3g})")
    assert delta > 0 and dev <= 4 * delta


def test_layout_epoch_range_composes(cluster_run):
    """Epochs n, n + 1, n + 2 in one call = three calls of one epoch, bit for bit (ping-pong parity included), 3-D."""
    from mmvae_amd import umap as U

    c = cluster_run
    g = [torch.from_numpy(t).cuda() for t in c["graph"]]
    y = torch.from_numpy(R.random_init(768, 3, 9).astype(np.float32)).cuda()
    kw = dict(n_epochs=EPOCHS, a=c["a"], b=c["b"], seed=SEED)
    three = U.optimize_layout(y, *g, first=7, count=3, **kw)
    two = U.optimize_layout(y, *g, first=7, count=2, **kw)
    step = y
    for n in (7, 8, 9):
        if n == 9:
            assert torch.equal(step, two)
        step = U.optimize_layout(step, *g, first=n, count=1, **kw)
    assert torch.equal(step, three) and not torch.equal(three, two)
    assert torch.equal(U.optimize_layout(y, *g, first=7, count=0, **kw), y)


def test_random_init_matches_the_mirror():
    from mmvae_amd import umap as U

    x = torch.zeros(333, 4, device="cuda")
    for C in (2, 3):
        y = U.initial_layout(x, C, "random", seed=12345).cpu().numpy()
        want = R.random_init(333, C, 12345)
        assert y.shape == (333, C) and np.abs(y - want).max() <= 2e-6 and np.abs(y).max() <= 10.0
    assert not np.array_equal(y, U.initial_layout(x, 3, "random", seed=12346).cpu().numpy())


@pytest.mark.parametrize("init, C", [("pca", 2), ("random", 2), ("pca", 3), ("random", 3)])
def test_umap_end_to_end(cluster_run, init, C):
    from sklearn.manifold import trustworthiness

    from mmvae_amd import umap as U

    c = cluster_run
    X, labels = c["X"], c["labels"]
    pptr, pind, psmp = c["graph"]
    if (init, C) == ("pca", 2):
        restated = c["final"]
    else:
        y0 = R.pca_init(X, C) if init == "pca" else R.random_init(len(X), C, SEED)
        restated, _ = R.optimize_layout(y0, pptr, pind, psmp, EPOCHS, c["a"], c["b"], SEED)
    floor = trustworthiness(X, restated, n_neighbors=K12, metric="cosine") - 0.01
    Xd = torch.from_numpy(X).cuda()
    kw = dict(n_neighbors=K12, n_components=C, n_epochs=EPOCHS, init=init)
    emb = U.umap_embeddings(Xd, seed=SEED, **kw)
    again = U.umap_embeddings(Xd, seed=SEED, n_jobs=2, low_memory=True, **kw)
    other = U.umap_embeddings(Xd, seed=SEED + 1, **kw)
    assert emb.is_cuda and emb.shape == (len(X), C) and emb.dtype == torch.float32
    assert bool(torch.isfinite(emb).all()) and bool(torch.isfinite(other).all())
    assert torch.equal(emb, again) and not torch.equal(emb, other)
    y = emb.cpu().numpy()
    trust = trustworthiness(X, y, n_neighbors=K12, metric="cosine")
    purity = R.label_purity(y, labels, K12)
    print(f"UMAP {init} {C}-D: trustworthiness {trust:.4f} (restatement {floor + 0.01:.4f}), label purity {purity:.4f}")
    assert trust >= floor and purity >= 0.99


def test_umap_refuses_what_it_does_not_implement():
    from mmvae_amd import umap as U

    x = torch.randn(64, 16, device="cuda")
    with pytest.raises(ValueError, match="cosine"):
        U.umap_embeddings(x, metric="euclidean")
    with pytest.raises(ValueError, match="n_components"):
        U.umap_embeddings(x, n_components=1)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        U.umap_embeddings(x.cpu())


def test_trainer_umap_and_h5_round_trip(tmp_path):
    from mmvae_amd import predictions as P
    from mmvae_amd.trainer import Trainer
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    model = MU.build_mirror(case, "cuda", str(tmp_path), use_engine=True)
    T = len(case["schedule"]) - 1
    MU.load_state(model, z, f"step{T}/sd/")
    x, _, _, _ = H.step_inputs(z, T)
    eid = str(z["eval/expert_id"])
    B = x.shape[0]
    rng = np.random.default_rng(2)
    batches = [((x * float(s)).cuda(), pd.DataFrame({"cell": [f"{j}_{i}" for i in range(B)]}), eid)
               for j, s in enumerate(rng.uniform(0.5, 1.5, 4))]
    emb, metadata = Trainer().umap(model, batches, n_neighbors=5, n_epochs=30, seed=3)
    assert emb.is_cuda and emb.shape == (4 * B, 2) and bool(torch.isfinite(emb).all())
    assert len(metadata) == 4 * B and metadata["cell"].tolist() == [f"{j}_{i}" for j in range(4) for i in range(B)]
    path = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(np.zeros((4 * B, 3), np.float32), metadata, path, "z")
    P.write_umap_embeddings(path, "z", emb)
    assert np.array_equal(P.load_from_hdf5(path, "z")[2], emb.cpu().numpy())
