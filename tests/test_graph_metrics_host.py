"""Host-side checks of graph connectivity and kBET (no GPU): the restatement itself against scipy, the C-ABI surface of
libmmvae_graph.so and its argument checks, the CPU-plumbing path of mmvae_amd.graph_metrics against the independent
restatement (tests/graph_restatement.py), the summary tables on a hand-made frame, and the command-line tool end to end
on a temporary directory.

Bounds.  Roots, counts and sizes are integers: equal.  stat is a sum of the same fp64 operations in the same order: equal.
pval: both sides run the same series / continued fraction; they differ in exp and log (torch's against libm's, a few
ulp each) whose argument reaches 745 at p = 1e-290 (a relative error of 745 * 2^-53 per ulp of the argument), and in up
to 60 accumulated terms: 2^-38 relative covers 745 * 8 * 2^-53 + 60 * 2^-53 = 6.7e-13 fivefold."""
import importlib.util
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import graph_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_graph.h")
P_REL = 2.0 ** -38

# reduced shapes of the GPU cases
KNN_COMPONENT_CASES = [(300, 16, 8, 5, 2.0), (700, 8, 4, 3, 1.0)]
KBET_CASES = [(200, 16, 16, 2), (300, 32, 31, 3), (300, 8, 64, 7)]


# --------------------------------------------------------------------------------------------- the restatement itself
def _scipy_roots(idx, codes):
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    src, dst = R.kept_edges(idx, codes)
    N = len(idx)
    n, label = csgraph.connected_components(sparse.coo_matrix((np.ones(len(src)), (src, dst)), shape=(N, N)), directed=False)
    first = np.full(n, N)
    np.minimum.at(first, label, np.arange(N))
    return first[label].astype(np.int32)


def test_restated_components_equal_scipys():
    cases = dict(R.hand_tables(n_path=500))
    cases["knn"] = R.knn_component_case(700, 8, 4, 3, 1.0)
    cases["random"] = (R.random_table(3000, 2), None, 1)
    for name, (idx, codes, _) in cases.items():
        assert np.array_equal(R.components(idx, codes), _scipy_roots(idx, codes)), name


def test_restated_p_values_equal_scipys():
    stats = pytest.importorskip("scipy.stats")
    for shape in KBET_CASES:
        idx, batch = R.kbet_case(*shape)
        stat, pval = R.kbet(idx, batch, shape[3])
        ok = ~np.isnan(pval)
        want = stats.chi2.sf(stat[ok], shape[3] - 1)
        assert (np.abs(pval[ok] - want) <= 1e-12 * want).all(), shape
    assert R.gamma_q(0.5, 0.5 * 3.841458820694124) == pytest.approx(0.05, rel=1e-12)


# ------------------------------------------------------------------------------------------------------- the C surface
def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _bind, _graph_lib

    declared = check_surface(_graph_lib.BINDING)
    assert set(declared) == {"mmvae_graph_abi_version", "mmvae_graph_build_arch", "mmvae_graph_cc_round_i32",
                             "mmvae_graph_component_sizes_i32", "mmvae_graph_kbet_f64"} == set(_graph_lib.GRAPH_PROTOTYPES)
    assert "_graph_lib" in _bind.MORE_DEVICE_LIBRARY_MODULES and "_graph_lib" not in _bind.DEVICE_LIBRARY_MODULES


def test_versions_and_constants():
    from mmvae_amd import _clust_lib, _graph_lib, _lib, _mix_lib, _sil_lib, _umap_lib, graph_metrics

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _graph_lib.load_graph()
    assert define("MMVAE_GRAPH_ABI_VERSION") == 1 == lib.mmvae_graph_abi_version() == _graph_lib.GRAPH_ABI_VERSION
    assert lib.mmvae_graph_build_arch() == b"gfx950"
    assert define("MMVAE_GRAPH_MAX_K") == _graph_lib.GRAPH_MAX_K == graph_metrics.MAX_K == _umap_lib.UMAP_MAX_K == 64
    assert define("MMVAE_GRAPH_MAX_BATCHES") == _graph_lib.GRAPH_MAX_BATCHES == graph_metrics.MAX_BATCHES == 64
    # the other libraries are untouched: same versions, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    others = [(_umap_lib.BINDING, _umap_lib.UMAP_PROTOTYPES), (_mix_lib.BINDING, _mix_lib.MIX_PROTOTYPES),
              (_sil_lib.BINDING, _sil_lib.BINDING.prototypes), (_clust_lib.BINDING, _clust_lib.BINDING.prototypes)]
    for binding, prototypes in others:
        assert getattr(binding.load(), binding.version_symbol)() == 1 == binding.abi_version
        assert not [n for n in prototypes if n.startswith("mmvae_graph_")]
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_graph_")]


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below carries the fake device address 16: had one of them launched, it would not return ERR_ARG."""
    from mmvae_amd import _graph_lib

    lib = _graph_lib.load_graph()
    #      N   k  idx codes parent changed stream
    ok = (100, 8, 16, 16, 16, 16, None)
    bad = {"N 0": {0: 0}, "N < 0": {0: -3}, "k 0": {1: 0}, "k 65": {1: 65}, "null idx": {2: None}, "null parent": {4: None},
           "null changed": {5: None}}
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_graph_cc_round_i32(*args) == _graph_lib.ERR_ARG, what
    #       N  root codes classes size_ws count largest n_comp stream
    oks = (100, 16, 16, 3, 16, 16, 16, 16, None)
    bads = {"N 0": {0: 0}, "N < 0": {0: -1}, "classes 0": {3: 0}, "no codes, two classes": {2: None, 3: 2}}
    bads.update({f"null argument {i}": {i: None} for i in (1, 4, 5, 6, 7)})
    for what, change in bads.items():
        args = [change.get(i, a) for i, a in enumerate(oks)]
        assert lib.mmvae_graph_component_sizes_i32(*args) == _graph_lib.ERR_ARG, what
    #       N   k  idx batch B freq dof stat pval stream
    okk = (100, 16, 16, 16, 3, 16, 2, 16, 16, None)
    badk = {"N 0": {0: 0}, "k 1": {1: 1}, "k 65": {1: 65}, "one batch": {4: 1, 6: 1}, "65 batches": {4: 65}, "dof 0": {6: 0},
            "dof = batches": {6: 3}, "dof < 0": {6: -1}}
    badk.update({f"null argument {i}": {i: None} for i in (2, 3, 5, 7, 8)})
    for what, change in badk.items():
        args = [change.get(i, a) for i, a in enumerate(okk)]
        assert lib.mmvae_graph_kbet_f64(*args) == _graph_lib.ERR_ARG, what


# ---------------------------------------------------------------------------------------------------- the python layer
def test_arguments_are_validated_before_any_launch():
    from mmvae_amd import backend, graph_metrics as G

    idx = torch.from_numpy(R.random_table(20, 4))
    codes = torch.zeros(20, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        G.connected_components(idx)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        G.kbet(idx, codes)
    with backend.cpu_plumbing():
        for wild in (20, -1):
            bad = idx.clone()
            bad[3, 2] = wild
            with pytest.raises(ValueError, match="neighbour indices"):
                G.connected_components(bad)
            with pytest.raises(ValueError, match="neighbour indices"):
                G.graph_connectivity(bad, codes, 1)
            with pytest.raises(ValueError, match="neighbour indices"):
                G.kbet(bad, codes, torch.tensor([0.5, 0.5]))
        with pytest.raises(ValueError, match="int32"):
            G.connected_components(idx.long())
        with pytest.raises(ValueError, match="int32"):
            G.connected_components(idx, codes.long())
        with pytest.raises(ValueError, match="int32"):
            G.kbet(idx, codes.long(), torch.tensor([0.5, 0.5]))
        with pytest.raises(ValueError, match=r"\[N, k\]"):
            G.connected_components(idx[0])
        with pytest.raises(ValueError, match="k <= 64"):
            G.connected_components(torch.zeros((3, 65), dtype=torch.int32))
        with pytest.raises(ValueError, match="2 <= k"):
            G.kbet(idx[:, :1], codes, torch.tensor([0.5, 0.5]))
        with pytest.raises(ValueError, match=r"must be \[N\]"):
            G.connected_components(idx, codes[:19])
        with pytest.raises(ValueError, match="max_rounds"):
            G.connected_components(idx, max_rounds=0)
        with pytest.raises(ValueError, match="n_batches"):
            G.kbet(idx, codes, torch.tensor([1.0]))
        with pytest.raises(ValueError, match="two batches"):
            G.kbet(idx, codes, torch.tensor([1.0, 0.0]))
        with pytest.raises(ValueError, match="two batches"):
            G.kbet(idx, codes)                      # every cell in batch 0
        with pytest.raises(ValueError, match="finite"):
            G.kbet(idx, codes - 1)                  # no cell in any batch
        with pytest.raises(ValueError, match="n_classes"):
            G.component_sizes(codes, None, 2)
        with pytest.raises(KeyError, match="tissue"):
            G.graph_metrics(torch.rand(20, 4), pd.DataFrame({"species": ["a"] * 20}), label_keys=("tissue",), n_neighbors=6)
        with pytest.raises(ValueError, match="metadata rows"):
            G.graph_metrics(torch.rand(20, 4), pd.DataFrame({"species": ["a"] * 19, "cell_type": ["b"] * 19}),
                            n_neighbors=6)


def _component_cases():
    cases = dict(R.hand_tables(n_path=512))
    for shape in KNN_COMPONENT_CASES:
        cases[f"knn {shape}"] = R.knn_component_case(*shape)
    cases["random"] = (R.random_table(5000, 8), None, 1)
    return cases


def test_cpu_components_equal_the_restatement():
    from mmvae_amd import backend, graph_metrics as G

    for name, (idx, codes, n_classes) in _component_cases().items():
        want = R.components(idx, codes)
        count, largest, n_comp = R.component_sizes(want, codes, n_classes)
        per, mean, _ = R.connectivity(idx, codes, n_classes)
        t_codes = None if codes is None else torch.from_numpy(codes)
        with backend.cpu_plumbing():
            root, rounds = G.connected_components(torch.from_numpy(idx), t_codes)
            got = G.component_sizes(root, t_codes, n_classes)
            if codes is not None:
                conn = G.graph_connectivity(torch.from_numpy(idx), t_codes, n_classes)
        assert root.dtype == torch.int32 and np.array_equal(root.numpy(), want), name
        assert 1 <= rounds <= G.MAX_ROUNDS, (name, rounds)
        assert np.array_equal(got[0].numpy(), count) and np.array_equal(got[1].numpy(), largest) and got[2] == n_comp, name
        if codes is not None:
            assert np.array_equal(conn.per_class.numpy(), per, equal_nan=True) and conn.score == mean, name
            assert conn.n_components == n_comp and conn.rounds == rounds
    # the hand-made answers
    cases = R.hand_tables(n_path=512)
    sizes = lambda name: R.component_sizes(R.components(*cases[name][:2]), cases[name][1], cases[name][2])  # noqa: E731
    assert sizes("cliques, one code")[1:] == ([64], 1) and sizes("cliques, no codes")[1:] == ([64], 1)
    assert sizes("cliques, two codes")[1].tolist() == [32, 32] and sizes("cliques, two codes")[2] == 2
    count, largest, n_comp = sizes("cliques, one end unlabelled")
    assert (count.tolist(), largest.tolist(), n_comp) == ([63], [32], 2)
    assert R.components(*cases["cliques, one end unlabelled"][:2])[32] == 32
    assert sizes("all self")[2] == 130 and sizes("star")[1:] == ([300], 1)
    # an empty class has no connectivity and is left out of the mean
    with backend.cpu_plumbing():
        conn = G.graph_connectivity(torch.from_numpy(cases["cliques, two codes"][0]),
                                    torch.from_numpy(cases["cliques, two codes"][1]), 3)
    assert conn.per_class.tolist()[:2] == [1.0, 1.0] and math.isnan(conn.per_class[2]) and conn.score == 1.0


def test_the_overlapping_mixture_is_not_fully_connected():
    idx, codes, n_classes = R.knn_component_case(*KNN_COMPONENT_CASES[1])
    per, mean, n_comp = R.connectivity(idx, codes, n_classes)
    assert (per < 1.0).any() and (per > 0.5).all() and n_comp > n_classes


def test_one_round_is_not_enough_for_a_path():
    from mmvae_amd import backend, graph_metrics as G

    idx = torch.from_numpy(R.path_table(64))
    with backend.cpu_plumbing():
        with pytest.raises(RuntimeError, match="max_rounds = 1"):
            G.connected_components(idx, max_rounds=1)
        root, rounds = G.connected_components(idx)
    assert int(root.max()) == 0 and 1 < rounds <= 13


def _p_close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool(((np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= P_REL * np.abs(want))).all())


def test_cpu_kbet_equals_the_restatement():
    from mmvae_amd import backend, graph_metrics as G

    for shape in KBET_CASES:
        idx, batch = R.kbet_case(*shape)
        stat, pval = R.kbet(idx, batch, shape[3])
        with backend.cpu_plumbing():
            got_stat, got_p, rejection = G.kbet(torch.from_numpy(idx), torch.from_numpy(batch))
        assert got_stat.dtype == got_p.dtype == torch.float64
        assert np.array_equal(got_stat.numpy(), stat, equal_nan=True), shape
        assert _p_close(got_p.numpy(), pval), shape
        assert rejection == R.rejection_rate(pval) and 0.2 < rejection < 0.995, (shape, rejection)
    for name, (idx, batch, freq, n_batches) in R.kbet_hand_cases().items():
        stat, pval = R.kbet(idx, batch, n_batches, freq)
        with backend.cpu_plumbing():
            got_stat, got_p, _ = G.kbet(torch.from_numpy(idx), torch.from_numpy(batch),
                                        None if freq is None else torch.from_numpy(freq))
        assert np.array_equal(got_stat.numpy(), stat, equal_nan=True), name
        assert _p_close(got_p.numpy(), pval), name
    # the hand-made answers: all from one batch, exactly at expectation, nobody labelled
    idx, batch, _, _ = R.kbet_hand_cases()["two batches"]
    stat, pval = R.kbet(idx, batch, 2)
    assert stat[0] == 4.0 == stat[3] and (stat[1], pval[1]) == (0.0, 1.0) and math.isnan(stat[2]) and math.isnan(pval[2])
    assert pval[0] == pytest.approx(math.erfc(math.sqrt(2.0)), rel=1e-14)  # Q(1/2, 2)
    assert (R.kbet(*[R.kbet_hand_cases()["a rare batch"][i] for i in (0, 1, 3, 2)])[1] <= 1e-280).all()


def test_kbet_per_label_on_cpu_plumbing():
    from mmvae_amd import backend, graph_metrics as G
    from mmvae_amd.umap import knn_graph

    X, label = R.mixture(21, 260, 6, 4)
    rng = np.random.default_rng(2)
    batch = rng.integers(0, 2, 260).astype(np.int32)
    X = X + 0.8 * rng.standard_normal((2, 6)).astype(np.float32)[batch]
    batch[label == 2] = 0                      # a class with one batch: skipped
    label[np.nonzero(label == 3)[0][6:]] = -1  # a class of six cells: skipped
    z, b, l = torch.from_numpy(X), torch.from_numpy(batch), torch.from_numpy(label)
    with backend.cpu_plumbing():
        per = G.kbet_per_label(z, b, l, n_labels=5)  # (class 4 is empty)
        want, k0s = [], []
        for c in (0, 1):
            rows = np.nonzero(label == c)[0]
            k0 = R.kbet_k0(batch[rows], 2)
            idx = knn_graph(z[rows], k0 + 1)[0].numpy()
            _, pval = R.kbet(idx, batch[rows], 2, R.batch_frequencies(batch[rows], 2))
            want.append(R.rejection_rate(pval))
            k0s.append(k0)
        with pytest.raises(ValueError, match="min_cells"):
            G.kbet_per_label(z, b, l, min_cells=2)
    assert per.tested.tolist() == [True, True, False, False, False] and per.k0.tolist() == k0s + [0, 0, 0]
    assert per.rejection.tolist()[:2] == want and bool(torch.isnan(per.rejection[2:]).all())
    assert per.score == pytest.approx(1.0 - sum(want) / 2, rel=1e-15)
    assert k0s == [min(63, max(10, int((label == c).sum() / 2 // 4)), int((label == c).sum()) - 2) for c in (0, 1)]


def test_summary_tables_on_a_hand_made_frame():
    from mmvae_amd import graph_metrics as G

    nan = float("nan")
    table = G.class_table(["B", "NK", "T", "none"], [40, 10, 50, 0], [40, 5, 45, 0], [10, 0, 12, 0], [0.25, nan, 0.75, nan],
                          [True, False, True, False])
    assert tuple(table.columns) == G.CLASS_COLUMNS and table["class"].tolist() == ["B", "NK", "T", "none"]
    assert table["connectivity"].tolist()[:3] == [1.0, 0.5, 0.9] and math.isnan(table["connectivity"][3])
    assert table["largest_component"].tolist() == [40, 5, 45, 0] and table["kbet_k0"].tolist() == [10, 0, 12, 0]
    row = G.summary_row("cell_type", table, 9, 4, 0.625)
    assert len(row) == len(G.SUMMARY_COLUMNS)
    got = dict(zip(G.SUMMARY_COLUMNS, row))
    assert got == {"column": "cell_type", "n_classes": 4, "n_cells": 100, "graph_connectivity": (1.0 + 0.5 + 0.9) / 3,
                   "n_components": 9, "cc_rounds": 4, "kbet_rejection_global": 0.625, "kbet_score": 0.5,
                   "n_classes_tested": 2}
    untested = G.summary_row("x", table.assign(kbet_tested=False), 9, 4, nan)
    assert math.isnan(untested[7]) and untested[8] == 0 and math.isnan(untested[6])


def _frame(n, species, cell_type):
    return pd.DataFrame({"species": species, "cell_type": cell_type, "cell": [f"c{i}" for i in range(n)]})


def _two_blobs(n=80):
    X, cluster = R.mixture(5, n, 6, 2, spread=0.3)
    species = np.where(np.arange(n) % 2 == 0, "human", "mouse").astype(object)
    cell_type = np.where(cluster == 0, "T", "B").astype(object)
    return X, cluster, species, cell_type


def test_graph_metrics_on_cpu_plumbing():
    from mmvae_amd import backend, graph_metrics as G

    X, cluster, species, cell_type = _two_blobs()
    cell_type[7] = np.nan
    with backend.cpu_plumbing():
        out = G.graph_metrics(torch.from_numpy(X), _frame(80, species, cell_type), n_neighbors=8)
        single = G.graph_metrics(torch.from_numpy(X), _frame(80, ["human"] * 80, cell_type), n_neighbors=8)
    assert out.columns == ("species", "cell_type") and out.idx.shape == (80, 8) and out.codes.shape == (2, 80)
    assert list(out.categories["cell_type"]) == ["B", "T"] and int(out.codes[1, 7]) == -1
    assert tuple(out.summary.columns) == G.SUMMARY_COLUMNS and len(out.summary) == 1
    idx, batch, label = out.idx.numpy(), out.codes[0].numpy(), out.codes[1].numpy()
    per, mean, n_comp = R.connectivity(idx, label, 2)
    row = out.summary.iloc[0]
    assert (row["column"], row["n_classes"], row["n_cells"], row["n_components"]) == ("cell_type", 2, 79, n_comp)
    assert row["graph_connectivity"] == mean and np.array_equal(out.root["cell_type"].numpy(), R.components(idx, label))
    stat, pval = R.kbet(idx, batch, 2)
    assert np.array_equal(out.kbet_stat.numpy(), stat) and _p_close(out.kbet_pval.numpy(), pval)
    assert row["kbet_rejection_global"] == R.rejection_rate(pval)
    table = out.per_class["cell_type"]
    assert tuple(table.columns) == G.CLASS_COLUMNS and table["class"].tolist() == ["B", "T"]
    assert table["connectivity"].tolist() == per.tolist() and table["kbet_tested"].tolist() == [True, True]
    assert row["n_classes_tested"] == 2 and row["kbet_score"] == pytest.approx(1.0 - table["kbet_rejection"].mean(), rel=1e-15)
    # the batches alternate inside the blobs: hardly a neighbourhood is rejected
    assert row["kbet_score"] > 0.8 and row["kbet_rejection_global"] < 0.2
    # one batch: the connectivity stands, kBET has nothing to test
    srow = single.summary.iloc[0]
    assert srow["graph_connectivity"] == mean and math.isnan(srow["kbet_score"]) and srow["n_classes_tested"] == 0
    assert single.kbet_pval is None and math.isnan(srow["kbet_rejection_global"])


def _tool():
    spec = importlib.util.spec_from_file_location("graph_metrics_tool", os.path.join(ROOT, "tools", "graph_metrics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_end_to_end_on_a_directory_and_an_h5(tmp_path, monkeypatch, capsys):
    from mmvae_amd import backend
    from mmvae_amd import predictions as P

    tool = _tool()
    monkeypatch.delenv("DIRECTORY", raising=False)
    X, cluster, species, cell_type = _two_blobs()
    meta = _frame(80, species, cell_type)
    meta["tissue"] = np.where(np.arange(80) < 40, "lung", "gut")
    np.savez(tmp_path / "z_embeddings.npz", embeddings=X.astype(np.float32))
    meta.to_pickle(tmp_path / "z_metadata.pkl")
    a = tool.parse_args(["--directory", str(tmp_path), "--keys", "z", "--labels", "cell_type", "--labels", "tissue"])
    assert (a.batch, a.labels, a.keys, a.save_dir, a.n_neighbors, a.alpha) == \
        ("species", ["cell_type", "tissue"], ["z"], None, 15, 0.05)
    assert tool.parse_args(["--directory", str(tmp_path), "--keys", "z"]).labels == ["cell_type"]
    with pytest.raises(SystemExit):
        tool.parse_args(["--directory", str(tmp_path / "absent"), "--keys", "z"])
    out_dir = tmp_path / "tables"
    with backend.cpu_plumbing():
        assert tool.main(["--directory", str(tmp_path), "--keys", "z", "--batch", "species", "--labels", "cell_type",
                          "--labels", "tissue", "--n_neighbors", "8", "--save_dir", str(out_dir)]) == 0
    printed = capsys.readouterr().out.split()
    names = ["graph_metrics.z.csv", "graph_metrics.z.cell_type.csv", "graph_metrics.z.tissue.csv"]
    assert printed == [str(out_dir / n) for n in names] and all(os.path.exists(p) for p in printed)
    table = pd.read_csv(out_dir / names[0])
    assert tuple(table.columns) == tuple(__import__("mmvae_amd.graph_metrics", fromlist=["x"]).SUMMARY_COLUMNS)
    assert table["column"].tolist() == ["cell_type", "tissue"] and table["n_cells"].tolist() == [80, 80]
    assert (table["graph_connectivity"] > 0.5).all() and (table["cc_rounds"] >= 1).all()
    assert pd.read_csv(out_dir / names[1])["class"].tolist() == ["B", "T"]
    # the predictions.h5 form: the same numbers next to the file
    h5 = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(X.astype(np.float32), meta, h5, "z")
    with backend.cpu_plumbing():
        assert tool.main(["--directory", h5, "--keys", "z", "--labels", "cell_type", "--n_neighbors", "8"]) == 0
    assert capsys.readouterr().out.split() == [str(tmp_path / names[0]), str(tmp_path / names[1])]
    again = pd.read_csv(tmp_path / names[0])
    assert again["graph_connectivity"][0] == table["graph_connectivity"][0] and again["kbet_score"][0] == table["kbet_score"][0]


def test_trainer_graph_metrics_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend, graph_metrics as G
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
        k = min(6, 2 * B - 1)
        batches = [(x, pd.DataFrame({"group": ["a"] * B, "donor": [f"d{i % 2}" for i in range(B)]}), eid),
                   (x.flip(0) * 0.5, pd.DataFrame({"group": ["b"] * B, "donor": [f"d{i % 2}" for i in range(B)]}), eid)]
        out = Trainer().graph_metrics(model, batches, batch_key="donor", label_keys=("group", "species"), n_neighbors=k)
    assert isinstance(out, G.GraphMetrics) and out.columns == ("donor", "group", "species")
    assert out.idx.shape == (2 * B, k) and out.codes.shape == (3, 2 * B) and out.kbet_pval.shape == (2 * B,)
    assert out.summary["column"].tolist() == ["group", "species"] and out.summary["n_classes"].tolist() == [2, 1]
    assert out.summary["n_cells"].tolist() == [2 * B, 2 * B] and set(out.root) == {"group", "species"}
    assert list(out.categories["species"]) == [eid] and len(out.per_class["species"]) == 1
