"""Host-side checks of the k-means clustering (no GPU): the C-ABI surface of libmmvae_clust.so and its argument checks,
the fp64 CPU-plumbing path of mmvae_amd.clustering against the independent restatement (tests/kmeans_restatement.py),
both against scikit-learn where that is installed, ARI and NMI, and the tables, the Trainer method and
`clusters_from_predictions` end to end on a temporary directory."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import kmeans_restatement as K
from tests import sil_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_clust.h")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _bind, _clust_lib

    declared = check_surface(_clust_lib.BINDING)
    assert set(declared) == {"mmvae_clust_abi_version", "mmvae_clust_build_arch", "mmvae_clust_kmeans_workspace_bytes",
                             "mmvae_clust_kmeans_step_f32", "mmvae_clust_seed_update_f32"} == set(_clust_lib.CLUST_PROTOTYPES)
    assert "_clust_lib" in _bind.MORE_DEVICE_LIBRARY_MODULES and "_clust_lib" not in _bind.DEVICE_LIBRARY_MODULES
    assert len(_bind.DEVICE_LIBRARY_MODULES) == 10


def test_versions_and_constants():
    from mmvae_amd import _clust_lib, _lib, _sil_lib, clustering

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _clust_lib.load_clust()
    assert define("MMVAE_CLUST_ABI_VERSION") == 1 == lib.mmvae_clust_abi_version() == _clust_lib.CLUST_ABI_VERSION
    assert lib.mmvae_clust_build_arch() == b"gfx950"
    assert define("MMVAE_CLUST_MAX_D") == _clust_lib.CLUST_MAX_D == clustering.MAX_D == 512
    assert define("MMVAE_CLUST_MAX_C") == _clust_lib.CLUST_MAX_C == clustering.MAX_C == 256
    assert define("MMVAE_CLUST_STATS_BYTES") == _clust_lib.CLUST_STATS_BYTES == clustering.STATS_BYTES == 24
    # the other libraries hold none of the new names
    assert not [n for n in list(_lib.PROTOTYPES) + list(_sil_lib.SIL_PROTOTYPES) if n.startswith("mmvae_clust_")]


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below carries the fake device address 16: had one of them launched, it would not return ERR_ARG."""
    from mmvae_amd import _clust_lib

    lib = _clust_lib.load_clust()
    size = lib.mmvae_clust_kmeans_workspace_bytes
    N, D, C = 100, 70, 3
    need = size(N, D, C)
    # 64 x 128 padded centroids, their norms; two workgroups (two row tiles) of 3 x 70 fp64 sums, 3 counts, an inertia and a
    # changed count, each table rounded up to 16 bytes; 3 shift2 shares
    assert need == 64 * 128 * 4 + 64 * 4 + 2 * 3 * 70 * 8 + 32 + 16 + 16 + 32
    for shape in ((0, 8, 1), (-1, 8, 1), (10, 0, 2), (10, -2, 2), (10, 513, 2), (10, 8, 0), (10, 8, -1), (10, 8, 11),
                  (1000, 8, 257)):
        assert size(*shape) == 0, shape
    for n in (1, 5, 64, 65, 1000, 100000, 1000000):
        for d in (1, 64, 65, 128, 129, 512):
            for c in (1, 15, 64, 65, 256):
                if c <= n:
                    assert size(n, d, c) > 0 and size(n, d, c) % 16 == 0 and size(n, d, c) <= (66 << 20), (n, d, c)
    #     N  D  x  ldx C centroids new label dist2 counts stats workspace bytes stream
    ok = (N, D, 16, D, C, 16, 16, 16, 16, 16, 16, 16, need, None)
    bad = {"N 0": {0: 0}, "N < 0": {0: -3}, "D 0": {1: 0, 3: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: D - 1},
           "C 0": {4: 0}, "C < 0": {4: -1}, "C > N": {4: N + 1}, "C 257": {0: 1000, 4: 257}, "short workspace": {12: need - 1},
           "no workspace": {12: 0}, "misaligned workspace": {11: 24}, "misaligned stats": {10: 20}}
    bad.update({f"null argument {i}": {i: None} for i in (2, 5, 6, 7, 8, 9, 10, 11)})
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_clust_kmeans_step_f32(*args) == _clust_lib.ERR_ARG, what
    #      N  D  x  ldx row first mind2 stream
    ok = (N, D, 16, D, 5, 1, 16, None)
    bad = {"N 0": {0: 0}, "D 0": {1: 0, 3: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: D - 1}, "row < 0": {4: -1},
           "row N": {4: N}, "no rows": {2: None}, "no mind2": {6: None}}
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_clust_seed_update_f32(*args) == _clust_lib.ERR_ARG, what


def _blobs(N, D, C, seed=5, spread=1.2):
    X, which = R.clusters(seed, N, D, C, spread=spread)
    return X, which


@pytest.mark.parametrize("N, D, C", [(5, 3, 2), (70, 8, 3), (150, 20, 6)])
def test_cpu_plumbing_step_and_seed_equal_the_restatement(N, D, C):
    from mmvae_amd import backend, clustering

    X, _ = _blobs(N, D, min(C, 4))
    rng = np.random.default_rng(N)
    cen = X[rng.choice(N, C, replace=False)] + 0.3 * rng.standard_normal((C, D))
    cen[C - 1] = cen[0]                      # a bit-equal copy: the tie goes to the smaller index, the later one is empty
    want = K.step(X, cen)
    t = torch.from_numpy
    with backend.cpu_plumbing():
        new, label, dist2, counts, stats = clustering.kmeans_step(t(X), t(cen))
        again = clustering.kmeans_step(t(X), t(cen), label)
        u = rng.random(C)
        rows = clustering.kmeans_seed(t(X), C, u)
        mind2 = clustering.seed_distances(t(X), 3)
        mind2 = clustering.seed_distances(t(X), 1, mind2)
    assert label.dtype == torch.int32 and counts.dtype == torch.int32 and new.dtype == torch.float64
    sure = want["lead"] > 1e-9
    assert np.array_equal(label.numpy()[sure], want["label"][sure]) and bool((label != C - 1).all())
    assert np.abs(dist2.numpy() - want["d2"]).max() <= 1e-10
    assert np.array_equal(counts.numpy(), want["counts"]) and counts[C - 1] == 0
    assert np.abs(new.numpy() - want["new"]).max() <= 1e-10 and np.array_equal(new.numpy()[C - 1], cen[C - 1])
    assert isinstance(stats, clustering.KMeansStats) and stats.changed == N and stats.empty == want["empty"] >= 1
    assert abs(stats.inertia - want["inertia"]) <= 1e-9 * want["inertia"]
    assert abs(stats.shift2 - want["shift2"]) <= 1e-9 * want["shift2"]
    assert again[4].changed == 0 and torch.equal(again[1], label)
    want_rows, margin = K.seed(X, C, u)
    assert margin > 1e-9 and rows.dtype == torch.int64 and np.array_equal(rows.numpy(), want_rows)
    assert len(set(rows.tolist())) == C
    e3, e1 = ((X - X[3]) ** 2).sum(1), ((X - X[1]) ** 2).sum(1)
    assert np.abs(mind2.numpy() - np.minimum(e3, e1)).max() <= 1e-10 and mind2[3] == 0 and mind2[1] == 0


def test_seeding_of_duplicated_rows_falls_back_to_rows_not_chosen():
    from mmvae_amd import backend, clustering

    X = np.zeros((6, 2))
    X[4:] = 1.0                               # two distinct points: rows 0 .. 3 and rows 4, 5
    u = np.array([0.0, 0.25, 0.9, 0.1])
    with backend.cpu_plumbing():
        rows = clustering.kmeans_seed(torch.from_numpy(X), 4, u)
    want, _ = K.seed(X, 4, u)
    assert rows.tolist() == want.tolist() == [0, 4, 1, 2]


@pytest.mark.parametrize("N, D, C, spread", [(70, 8, 3, 0.2), (300, 12, 5, 0.2), (200, 6, 4, 3.0)])
def test_cpu_plumbing_fit_equals_the_restatement(N, D, C, spread):
    from mmvae_amd import backend, clustering

    X, which = _blobs(N, D, C, seed=11, spread=spread)
    want = K.fit(X, C, seed_value=3, n_init=2, max_iter=100)
    with backend.cpu_plumbing():
        got = clustering.kmeans_fit(torch.from_numpy(X), C, seed=3, n_init=2, max_iter=100)
    assert isinstance(got, clustering.KMeansResult) and got.labels.dtype == torch.int32 and got.centroids.dtype == torch.float64
    assert want["min_lead"] > 1e-9
    assert np.array_equal(got.labels.numpy(), want["labels"]) and got.n_iter == want["n_iter"]
    assert got.converged == want["converged"] is True
    assert np.abs(got.centroids.numpy() - want["centroids"]).max() <= 1e-10
    assert abs(got.inertia - want["inertia"]) <= 1e-9 * want["inertia"]
    assert np.array_equal(got.counts.numpy(), want["counts"]) and int(got.counts.sum()) == N
    assert np.allclose(got.history, want["history"], rtol=1e-9, atol=0) and len(got.history) == got.n_iter
    assert all(b <= a * (1 + 1e-12) for a, b in zip(got.history, got.history[1:]))


def test_fit_relocates_an_empty_cluster_as_the_restatement_does():
    """Three tight blobs and four clusters seeded so that two seeds are bit-equal rows: the later one starts empty."""
    from mmvae_amd import backend, clustering

    X, _ = _blobs(90, 4, 3, seed=2, spread=0.1)
    X[1] = X[0]
    Xc = K.centred(X, False)
    cen = Xc[[0, 1, 40, 80]]
    s = K.step(Xc, cen)
    assert s["empty"] == 1 and s["counts"][1] == 0
    K.relocate(Xc, s["new"], s["counts"], s["d2"])
    far = int(np.argmax(s["d2"]))
    assert np.array_equal(s["new"][1], Xc[far])
    with backend.cpu_plumbing():
        new, label, dist2, counts, stats = clustering.kmeans_step(torch.from_numpy(Xc), torch.from_numpy(cen))
        assert stats.empty == 1
        clustering._relocate(new, counts, dist2, torch.from_numpy(Xc))
    assert np.array_equal(new.numpy()[1], Xc[far])


def test_fit_equals_scikit_learn_on_separate_clusters():
    cluster = pytest.importorskip("sklearn.cluster")
    from mmvae_amd import backend, clustering

    for N, D, C in ((300, 12, 5), (500, 30, 8)):
        X, which = _blobs(N, D, C, seed=21, spread=0.3)
        want = K.fit(X, C, seed_value=1)
        Xc = want["Xc"]
        km = cluster.KMeans(n_clusters=C, init=Xc[want["seed_rows"]], n_init=1, algorithm="lloyd").fit(Xc)
        with backend.cpu_plumbing():
            got = clustering.kmeans_fit(torch.from_numpy(X), C, seed=1)
        for labels, inertia in ((want["labels"], want["inertia"]), (got.labels.numpy(), got.inertia)):
            assert np.array_equal(labels, km.labels_)
            assert abs(inertia - km.inertia_) <= 1e-9 * km.inertia_
        assert np.abs(got.centroids.numpy() - (km.cluster_centers_ + X.mean(0))).max() <= 1e-9


def _partitions():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 5, 400)
    noisy = np.where(rng.random(400) < 0.3, rng.integers(0, 4, 400), a % 4)
    unlabelled = noisy.copy()
    unlabelled[rng.random(400) < 0.1] = -1
    return {"noisy": (a, noisy), "identical": (a, a.copy()), "renamed": (a, (a + 2) % 5), "single cluster": (np.zeros(400, int), a),
            "both single": (np.zeros(400, int), np.ones(400, int)), "independent": (a, rng.integers(0, 3, 400)),
            "singletons": (np.arange(400), a), "unlabelled": (a, unlabelled)}


def test_ari_and_nmi_equal_scikit_learn_and_the_restatement():
    from mmvae_amd import clustering

    metrics = None
    try:
        from sklearn import metrics
    except ImportError:
        pass
    t = torch.from_numpy
    for name, (a, b) in _partitions().items():
        table = clustering.contingency(t(a), t(b))
        assert table.dtype == torch.int64 and np.array_equal(table.numpy(), K.table_of(a, b)), name
        ari, nmi = clustering.adjusted_rand_index(table), clustering.normalized_mutual_info(table)
        assert abs(ari - K.ari(a, b)) <= 1e-12 and abs(nmi - K.nmi(a, b)) <= 1e-12, name
        if metrics is not None:
            keep = (a >= 0) & (b >= 0)
            assert abs(ari - metrics.adjusted_rand_score(b[keep], a[keep])) <= 1e-12, name
            assert abs(nmi - metrics.normalized_mutual_info_score(b[keep], a[keep])) <= 1e-12, name
    a, b = _partitions()["unlabelled"]
    assert int(clustering.contingency(t(a), t(b)).sum()) == int((b >= 0).sum()) < 400
    same = clustering.contingency(t(a), t(a))
    assert clustering.adjusted_rand_index(same) == 1.0 and abs(clustering.normalized_mutual_info(same) - 1.0) <= 1e-12
    single = clustering.contingency(t(np.zeros(400, int)), t(a))
    assert clustering.adjusted_rand_index(single) == 0.0 and clustering.normalized_mutual_info(single) <= 1e-15
    empty = clustering.contingency(t(np.full(4, -1)), t(np.zeros(4, int)), 2, 3)
    assert empty.shape == (2, 3) and math.isnan(clustering.adjusted_rand_index(empty))
    assert math.isnan(clustering.normalized_mutual_info(empty))
    wide = clustering.contingency(t(a), t(b), 7, 6)
    assert wide.shape == (7, 6) and clustering.adjusted_rand_index(wide) == clustering.adjusted_rand_index(
        clustering.contingency(t(a), t(b)))
    with pytest.raises(ValueError, match="exceeds"):
        clustering.contingency(t(a), t(b), 2, 6)
    with pytest.raises(TypeError, match="int32 or int64"):
        clustering.contingency(t(a).float(), t(b))


def test_cpu_tensors_are_refused_outside_cpu_plumbing_and_arguments_are_validated():
    from mmvae_amd import backend, clustering

    X, which = _blobs(20, 4, 2)
    x = torch.from_numpy(X)
    frame = pd.DataFrame({"cell_type": ["x", "y"] * 10})
    for call in (lambda: clustering.kmeans_step(x, x[:2]), lambda: clustering.kmeans_seed(x, 2, [0.1, 0.2]),
                 lambda: clustering.kmeans_fit(x, 2), lambda: clustering.cluster_metrics(x, frame),
                 lambda: clustering.seed_distances(x, 0)):
        with pytest.raises(RuntimeError, match="cpu_plumbing"):
            call()
    with backend.cpu_plumbing():
        with pytest.raises(ValueError, match="D <= 512"):
            clustering.kmeans_fit(torch.zeros(20, 513), 2)
        with pytest.raises(ValueError, match="n_clusters"):
            clustering.kmeans_fit(x, 21)
        with pytest.raises(ValueError, match="n_clusters"):
            clustering.kmeans_fit(torch.zeros(300, 2), 257)
        with pytest.raises(ValueError, match="centroids must be"):
            clustering.kmeans_step(x, x[:2, :3])
        with pytest.raises(ValueError, match="label must be"):
            clustering.kmeans_step(x, x[:2], torch.zeros(20, dtype=torch.int64))
        with pytest.raises(ValueError, match="uniforms"):
            clustering.kmeans_seed(x, 2, [0.1, 1.0])
        with pytest.raises(ValueError, match="row must be"):
            clustering.seed_distances(x, 20)
        with pytest.raises(KeyError, match="tissue"):
            clustering.cluster_metrics(x, frame, label_keys=("tissue",))
        with pytest.raises(ValueError, match="metadata rows"):
            clustering.cluster_metrics(x, frame[:19])


def _three_clusters(n=90, seed=9):
    X, cluster = R.clusters(seed, n, 6, 3, spread=0.1)
    cell_type = np.array(["B", "NK", "T"], dtype=object)[cluster]
    tissue = np.where(np.arange(n) < n // 2, "lung", "gut").astype(object)
    return X, cluster, pd.DataFrame({"cell_type": cell_type, "tissue": tissue})


def test_cluster_metrics_on_cpu_plumbing():
    from mmvae_amd import backend, clustering

    X, cluster, meta = _three_clusters()
    meta.loc[7, "cell_type"] = np.nan
    with backend.cpu_plumbing():
        out = clustering.cluster_metrics(torch.from_numpy(X), meta, label_keys=("cell_type", "tissue"), seed=4)
        capped = clustering.cluster_metrics(torch.from_numpy(X), meta, n_clusters=1000, max_iter=2)
    assert out.columns == ("cell_type", "tissue") and out.codes.shape == (2, 90) and out.codes.dtype == torch.int32
    assert tuple(out.summary.columns) == clustering.SUMMARY_COLUMNS and out.summary["column"].tolist() == ["cell_type", "tissue"]
    assert out.summary["n_clusters"].tolist() == [3, 2] and out.summary["n_cells"].tolist() == [89, 90]
    label = out.codes[0].numpy()
    assert label[7] == -1 and np.array_equal(np.delete(label, 7), np.delete(cluster, 7))
    for n, (key, C) in enumerate((("cell_type", 3), ("tissue", 2))):
        want = K.fit(X, C, seed_value=4)
        fit = out.fits[key]
        assert np.array_equal(fit.labels.numpy(), want["labels"]) and fit.n_iter == want["n_iter"]
        codes = out.codes[n].numpy()
        table = out.contingency[key]
        assert np.array_equal(table.values, K.table_of(want["labels"], codes)) and table.index.name == "cluster"
        assert table.columns.tolist() == list(out.categories[key])
        assert abs(out.summary["nmi"][n] - K.nmi(want["labels"], codes)) <= 1e-12
        assert abs(out.summary["ari"][n] - K.ari(want["labels"], codes)) <= 1e-12
        assert abs(out.summary["inertia"][n] - want["inertia"]) <= 1e-9 * want["inertia"] and out.summary["converged"][n]
    assert out.summary["ari"][0] == 1.0 and abs(out.summary["nmi"][0] - 1.0) <= 1e-12   # three tight blobs are recovered
    assert out.summary["ari"][1] < 0.5                                                    # the tissue is no cluster
    assert capped.summary["n_clusters"].tolist() == [90] and capped.fits["cell_type"].counts.shape == (90,)


def test_tables_and_clusters_from_predictions(tmp_path):
    from mmvae_amd import backend, clustering
    from mmvae_amd import predictions as P

    X, cluster, meta = _three_clusters(60)
    np.savez(tmp_path / "z_embeddings.npz", embeddings=X.astype(np.float32))
    meta.to_pickle(tmp_path / "z_metadata.pkl")
    out_dir = tmp_path / "tables"
    with backend.cpu_plumbing():
        paths = clustering.clusters_from_predictions(str(tmp_path), ("z",), ("cell_type", "tissue"), save_dir=str(out_dir),
                                                     seed=2)
        direct = clustering.cluster_metrics(torch.from_numpy(X.astype(np.float32)), meta, ("cell_type", "tissue"), seed=2)
    names = ["clusters.z.csv", "clusters.z.cell_type.contingency.csv", "clusters.z.cell_type.labels.npy",
             "clusters.z.tissue.contingency.csv", "clusters.z.tissue.labels.npy"]
    assert paths == [str(out_dir / n) for n in names] and all(os.path.exists(p) for p in paths)
    table = pd.read_csv(out_dir / names[0])
    assert tuple(table.columns) == clustering.SUMMARY_COLUMNS and table["column"].tolist() == ["cell_type", "tissue"]
    assert np.allclose(table["ari"], direct.summary["ari"], rtol=0, atol=1e-12) and table["ari"][0] == 1.0
    cont = pd.read_csv(out_dir / names[1], index_col=0)
    assert cont.columns.tolist() == ["B", "NK", "T"] and cont.index.tolist() == [0, 1, 2] and int(cont.values.sum()) == 60
    labels = np.load(out_dir / names[2])
    assert labels.dtype == np.int32 and np.array_equal(labels, direct.fits["cell_type"].labels.numpy())
    assert K.ari(labels, cluster) == 1.0
    # the predictions.h5 form: the files next to the file
    h5 = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(X.astype(np.float32), meta, h5, "z")
    with backend.cpu_plumbing():
        again = clustering.clusters_from_predictions(h5, ("z",), seed=2)
        with pytest.raises(KeyError):
            clustering.clusters_from_predictions(h5, ("absent",))
    assert again == [str(tmp_path / n) for n in names[:3]]
    assert np.array_equal(np.load(tmp_path / names[2]), labels)


def test_trainer_cluster_metrics_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend, clustering
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
        batches = [(x, pd.DataFrame({"group": ["a"] * B}), eid), (x.flip(0) * 0.5, pd.DataFrame({"group": ["b"] * B}), eid)]
        out = Trainer().cluster_metrics(model, batches, label_keys=("group",), seed=1)
        with pytest.raises(ValueError, match="no batches"):
            Trainer().cluster_metrics(model, [])
    assert isinstance(out, clustering.ClusterMetrics) and out.codes.shape == (1, 2 * B)
    assert out.fits["group"].labels.shape == (2 * B,) and int(out.fits["group"].counts.sum()) == 2 * B
    assert out.summary["n_clusters"].tolist() == [2] and out.summary["n_cells"].tolist() == [2 * B]
    assert np.isfinite(out.summary[["nmi", "ari", "inertia"]].values.astype(float)).all()
    assert 0.0 <= out.summary["nmi"][0] <= 1.0 and -1.0 <= out.summary["ari"][0] <= 1.0
