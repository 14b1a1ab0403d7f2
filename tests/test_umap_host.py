"""Host-side checks of the UMAP library (no GPU): the C-ABI surface of libmmvae_umap.so, find_ab_params against
umap-learn's published values, the activity schedule, the fp64 CPU-plumbing path against the independent restatement
(tests/umap_restatement.py), and the predictions.h5 round trip of the embedding."""
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import umap_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_umap.h")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _umap_lib

    declared = check_surface(_umap_lib.BINDING)
    assert set(declared) == {"mmvae_umap_abi_version", "mmvae_umap_build_arch", "mmvae_umap_knn_cosine_workspace_bytes",
                             "mmvae_umap_knn_cosine_f32", "mmvae_umap_smooth_knn_f32", "mmvae_umap_random_init_f32",
                             "mmvae_umap_layout_f32"} == set(_umap_lib.UMAP_PROTOTYPES)


def test_versions_and_arch():
    from mmvae_amd import _lib, _umap_lib

    header = open(HEADER).read()
    assert int(re.search(r"#define\s+MMVAE_UMAP_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    lib = _umap_lib.load_umap()
    assert lib.mmvae_umap_abi_version() == 1 == _umap_lib.UMAP_ABI_VERSION
    assert lib.mmvae_umap_build_arch() == b"gfx950"
    assert int(re.search(r"#define\s+MMVAE_UMAP_MAX_K\s+(\d+)", header).group(1)) == _umap_lib.UMAP_MAX_K
    assert int(re.search(r"#define\s+MMVAE_UMAP_MAX_D\s+(\d+)", header).group(1)) == _umap_lib.UMAP_MAX_D
    # the training library is untouched: same version, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_umap_")]


def test_workspace_helper_and_argument_checks():
    from mmvae_amd import _umap_lib

    lib = _umap_lib.load_umap()
    need = lib.mmvae_umap_knn_cosine_workspace_bytes
    for N, D, k in ((16, 8, 16), (16, 8, 17), (300, 128, 1), (300, 128, 65), (300, 513, 30), (300, 0, 30), (2, 8, 2)):
        assert need(N, D, k) == 0, (N, D, k)
        assert lib.mmvae_umap_knn_cosine_f32(N, D, k, 16, max(D, 1), 16, 16, 16, 1 << 30, None) == _umap_lib.ERR_ARG
    for N, D, k in ((3, 1, 2), (16, 8, 15), (300, 128, 64), (100000, 128, 30), (5000, 512, 30)):
        nbytes = need(N, D, k)
        assert nbytes > 0 and nbytes % 16 == 0 and nbytes <= 4 * (N + 127) * max(2 * D, 64), (N, D, k, nbytes)
    # null pointers, a short leading dimension, a short workspace, a bad epoch range: refused before any launch
    assert lib.mmvae_umap_knn_cosine_f32(300, 128, 30, None, 128, 16, 16, 16, 1 << 30, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_knn_cosine_f32(300, 128, 30, 16, 127, 16, 16, 16, 1 << 30, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_knn_cosine_f32(300, 128, 30, 16, 128, 16, 16, 16, 64, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_layout_f32(10, 4, 16, 16, 16, 16, 32, 1.0, 1.0, 1.0, 200, 1, 1, 0, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_layout_f32(10, 2, 16, 16, 16, 16, 32, 1.0, 1.0, 1.0, 200, 200, 2, 0, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_layout_f32(10, 2, 16, 16, 16, 16, 16, 1.0, 1.0, 1.0, 200, 1, 1, 0, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_smooth_knn_f32(10, 65, 16, 16, 16, 16, 16, 16, None) == _umap_lib.ERR_ARG
    assert lib.mmvae_umap_random_init_f32(0, 16, 0, None) == _umap_lib.ERR_ARG


@pytest.mark.parametrize("args, want", [((1.0, 0.1), (1.576943, 0.895061)), ((1.0, 0.3), (0.992176, 1.112253))])
def test_find_ab_params(args, want):
    from mmvae_amd import umap as U

    a, b = U.find_ab_params(*args)
    assert abs(a - want[0]) <= 1e-5 and abs(b - want[1]) <= 1e-5, (a, b)
    ra, rb = R.find_ab_params(*args)
    assert abs(ra - want[0]) <= 1e-5 and abs(rb - want[1]) <= 1e-5, (ra, rb)


def test_activity_schedule_fires_each_edge_its_sample_count():
    for n_epochs in (1, 7, 200, 500):
        samples = np.arange(1, n_epochs + 1)
        fired = np.zeros(n_epochs, dtype=np.int64)
        for n in range(1, n_epochs + 1):
            fired += R.active(n, samples, n_epochs)
        assert np.array_equal(fired, samples), n_epochs
    assert R.active(1, np.array([200]), 200).all() and not R.active(1, np.array([199]), 200).any()


def _small_problem():
    X, labels = R.clusters(seed=3, n_clusters=4, per=24, dim=12)
    X[5] = X[4]      # a duplicate
    X[17] = 0.0      # a zero row
    return X, labels


def test_cpu_plumbing_matches_the_restatement():
    from mmvae_amd import backend
    from mmvae_amd import umap as U

    X, _ = _small_problem()
    k, n_epochs, seed = 10, 30, 5
    ridx, rdist, _ = R.cosine_knn(X, k)
    rsigma, rrho = R.smooth_knn_dist(rdist)
    rw = R.membership_strengths(ridx, rdist, rrho, rsigma)
    rptr, rind, rdata = R.symmetrise(ridx, rw)
    pptr, pind, psmp = R.prune_and_samples(rptr, rind, rdata, n_epochs)
    a, b = R.find_ab_params(1.0, 0.3)
    with backend.cpu_plumbing():
        Xt = torch.from_numpy(X)
        idx, dist = U.knn_graph(Xt, k)
        assert idx.dtype == torch.int32 and dist.dtype == torch.float64
        assert np.abs(dist.numpy() - rdist).max() <= 1e-12
        gaps = np.diff(rdist, axis=1)
        firm = np.ones_like(ridx, dtype=bool)
        firm[:, 1:] &= gaps > 1e-9
        firm[:, :-1] &= gaps > 1e-9
        assert np.array_equal(idx.numpy()[firm], ridx[firm]) and firm.mean() > 0.9
        assert (idx[:, 0].numpy() == np.arange(len(X))).all() and (dist[:, 0] == 0).all()
        assert dist[4, 1] <= 1e-12 and idx[4, 1] == 5 and (dist[17, 1:] == 1.0).all()
        g = U.fuzzy_simplicial_set(torch.from_numpy(ridx.astype(np.int32)), torch.from_numpy(rdist))
        assert np.abs(g.rho.numpy() - rrho).max() == 0 and np.abs(g.sigma.numpy() - rsigma).max() <= 1e-12
        assert np.abs(g.memberships.numpy() - rw).max() <= 1e-12
        assert np.array_equal(g.indptr.numpy(), rptr) and np.array_equal(g.indices.numpy(), rind)
        assert np.abs(g.data.numpy() - rdata).max() <= 1e-12
        ptr, ind, smp = U.layout_graph(g, n_epochs)
        assert np.array_equal(ptr.numpy(), pptr) and np.array_equal(ind.numpy(), pind) and np.array_equal(smp.numpy(), psmp)
        for init, C in (("pca", 2), ("random", 3)):
            y0 = U.initial_layout(Xt, C, init, seed)
            ry0 = R.pca_init(X, C) if init == "pca" else R.random_init(len(X), C, seed)
            assert np.abs(y0.numpy() - ry0).max() <= 1e-9 and np.abs(ry0).max() <= 10.0
            one = U.optimize_layout(y0, ptr, ind, smp, n_epochs=n_epochs, a=a, b=b, seed=seed, first=1, count=1)
            want = R.layout_epoch(ry0, pptr, pind, psmp, 1, n_epochs, a, b, seed)
            assert np.abs(one.numpy() - want).max() <= 1e-9
            mid = U.optimize_layout(torch.from_numpy(want), ptr, ind, smp, n_epochs=n_epochs, a=a, b=b, seed=seed, first=2,
                                    count=2)
            want3 = R.layout_epoch(R.layout_epoch(want, pptr, pind, psmp, 2, n_epochs, a, b, seed), pptr, pind, psmp, 3,
                                   n_epochs, a, b, seed)
            assert np.abs(mid.numpy() - want3).max() <= 1e-8
        emb = U.umap_embeddings(Xt, n_neighbors=k, n_epochs=n_epochs, seed=seed, low_memory=True, n_jobs=3, verbose=False)
        assert emb.shape == (len(X), 2) and bool(torch.isfinite(emb).all())


def test_negatives_are_in_range_and_differ_between_epochs_and_seeds():
    slots = np.arange(1000)
    a, b, c = R.negatives(slots, 1, 768, 0), R.negatives(slots, 2, 768, 0), R.negatives(slots, 1, 768, 1)
    assert a.shape == (1000, 5) and a.min() >= 0 and a.max() < 768
    assert (a != b).mean() > 0.9 and (a != c).mean() > 0.9
    assert np.array_equal(a, R.negatives(slots, 1, 768, 0))


def test_arguments_are_validated():
    from mmvae_amd import backend
    from mmvae_amd import umap as U

    x = torch.rand(20, 6)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        U.umap_embeddings(x, n_neighbors=5)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        U.knn_graph(x, 5)
    with backend.cpu_plumbing():
        with pytest.raises(ValueError, match="cosine"):
            U.umap_embeddings(x, n_neighbors=5, metric="euclidean")
        with pytest.raises(ValueError, match="n_components"):
            U.umap_embeddings(x, n_neighbors=5, n_components=4)
        with pytest.raises(ValueError, match="n_neighbors"):
            U.knn_graph(x, 20)
        with pytest.raises(ValueError, match="n_neighbors"):
            U.knn_graph(x, 65)
        with pytest.raises(ValueError, match="spectral"):
            U.umap_embeddings(x, n_neighbors=5, init="spectral")


def test_umap_embeddings_h5_round_trip(tmp_path):
    from mmvae_amd import predictions as P

    path = str(tmp_path / "predictions.h5")
    rng = np.random.default_rng(0)
    z = rng.standard_normal((9, 4)).astype(np.float32)
    md = pd.DataFrame({"cell": [f"c{i}" for i in range(9)], "n": np.arange(9)})
    with pytest.raises(FileNotFoundError):
        P.write_umap_embeddings(path, "z", z[:, :2])
    P.save_to_hdf5(z, md, path, "z")
    assert P.load_from_hdf5(path, "z")[2] is None
    with pytest.raises(KeyError):
        P.write_umap_embeddings(path, "other", z[:, :2])
    first = rng.standard_normal((9, 2)).astype(np.float32)
    P.write_umap_embeddings(path, "z", torch.from_numpy(first))
    data, meta, emb = P.load_from_hdf5(path, "z")
    assert emb.dtype == np.float32 and np.array_equal(emb, first) and np.array_equal(data, z) and len(meta) == 9
    second = rng.standard_normal((9, 3))  # replaced, with another width and float type
    P.write_umap_embeddings(path, "z", second)
    data, meta, emb = P.load_from_hdf5(path, "z")
    assert emb.dtype == np.float64 and np.array_equal(emb, second) and np.array_equal(data, z)
    P.save_to_hdf5(z, md, path, "z")  # the predictions still append next to it
    assert P.load_from_hdf5(path, "z")[0].shape == (18, 4)


def test_trainer_umap_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend
    from mmvae_amd import predictions as P
    from mmvae_amd.trainer import Trainer
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    with backend.cpu_plumbing():
        model = MU.build_mirror(case, "cpu", str(tmp_path), use_engine=True)
        T = len(case["schedule"]) - 1
        MU.load_state(model, z, f"step{T}/sd/")
        x, _, _, _ = H.step_inputs(z, T)
        eid = str(z["eval/expert_id"])
        B = x.shape[0]
        batches = [(x, pd.DataFrame({"cell": [f"a{i}" for i in range(B)]}), eid),
                   (x.flip(0) * 0.5, pd.DataFrame({"cell": [f"b{i}" for i in range(B)]}), eid)]
        emb, metadata = Trainer().umap(model, batches, n_neighbors=min(5, 2 * B - 1), n_epochs=20, seed=1)
    assert emb.shape == (2 * B, 2) and len(metadata) == 2 * B and bool(torch.isfinite(emb).all())
    assert metadata["cell"].tolist() == [f"a{i}" for i in range(B)] + [f"b{i}" for i in range(B)]
    assert (metadata["species"] == eid).all()
    path = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(np.zeros((2 * B, 3), np.float32), metadata, path, "z")
    P.write_umap_embeddings(path, "z", emb)
    assert np.array_equal(P.load_from_hdf5(path, "z")[2], emb.numpy())
