"""Host-side checks of the integration metrics (no GPU): the C-ABI surface of libmmvae_mix.so and its argument checks,
the fp64 CPU-plumbing path of mmvae_amd.mixing against the independent restatement (tests/mix_restatement.py), the
summary tables on hand-made cases, and the command-line tool end to end on a temporary directory."""
import importlib.util
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import mix_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_mix.h")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _bind, _mix_lib

    declared = check_surface(_mix_lib.BINDING)
    assert set(declared) == {"mmvae_mix_abi_version", "mmvae_mix_build_arch", "mmvae_mix_calibrate_f32",
                             "mmvae_mix_lisi_f32", "mmvae_mix_transfer_f32"} == set(_mix_lib.MIX_PROTOTYPES)
    assert "_mix_lib" in _bind.DEVICE_LIBRARY_MODULES


def test_versions_and_constants():
    from mmvae_amd import _lib, _mix_lib, _umap_lib, mixing

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _mix_lib.load_mix()
    assert define("MMVAE_MIX_ABI_VERSION") == 1 == lib.mmvae_mix_abi_version() == _mix_lib.MIX_ABI_VERSION
    assert lib.mmvae_mix_build_arch() == b"gfx950"
    assert define("MMVAE_MIX_MAX_K") == _mix_lib.MIX_MAX_K == mixing.MAX_K == _umap_lib.UMAP_MAX_K == 64
    assert define("MMVAE_MIX_MAX_COLS") == _mix_lib.MIX_MAX_COLS == mixing.MAX_COLS == 8
    # the training library and the UMAP library are untouched: same versions, none of the new names
    assert _lib.load().mmvae_abi_version() == 16 and _umap_lib.load_umap().mmvae_umap_abi_version() == 1
    assert not [n for n in list(_lib.PROTOTYPES) + list(_umap_lib.UMAP_PROTOTYPES) if n.startswith("mmvae_mix_")]


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below carries the fake device address 16: had one of them launched, it would not return ERR_ARG."""
    from mmvae_amd import _mix_lib

    lib = _mix_lib.load_mix()
    nan = float("nan")
    #      N   k  idx dist perplexity beta tries stream
    ok = (100, 16, 16, 16, 5.0, 16, 16, None)
    bad = {"N 0": {0: 0}, "N < 0": {0: -3}, "k 2": {1: 2, 4: 1.5}, "k 65": {1: 65, 4: 21.0}, "perplexity 1": {4: 1.0},
           "perplexity k - 1": {4: 15.0}, "perplexity > k - 1": {4: 40.0}, "perplexity 0": {4: 0.0}, "perplexity nan": {4: nan},
           "null idx": {2: None}, "null dist": {3: None}, "null beta": {5: None}, "null tries": {6: None}}
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_mix_calibrate_f32(*args) == _mix_lib.ERR_ARG, what
    #       N   k  idx dist beta cols codes ldc lisi ldl stream
    okl = (100, 16, 16, 16, 16, 3, 16, 100, 16, 100, None)
    badl = {"N 0": {0: 0}, "k 2": {1: 2}, "k 65": {1: 65}, "cols 0": {5: 0}, "cols 9": {5: 9}, "ldc < N": {7: 99},
            "ldl < N": {9: 99}, "null idx": {2: None}, "null dist": {3: None}, "null beta": {4: None},
            "null codes": {6: None}, "null lisi": {8: None}}
    for what, change in badl.items():
        args = [change.get(i, a) for i, a in enumerate(okl)]
        assert lib.mmvae_mix_lisi_f32(*args) == _mix_lib.ERR_ARG, what
    #       N   k  idx dist beta batch label pred conf cross stream
    okt = (100, 16, 16, 16, 16, 16, 16, 16, 16, 16, None)
    badt = {"N 0": {0: 0}, "k 2": {1: 2}, "k 65": {1: 65}}
    badt.update({f"null argument {i}": {i: None} for i in range(2, 10)})
    for what, change in badt.items():
        args = [change.get(i, a) for i, a in enumerate(okt)]
        assert lib.mmvae_mix_transfer_f32(*args) == _mix_lib.ERR_ARG, what


# (input, N, dim, k, perplexity)
CPU_CASES = [("gaussian", 70, 8, 64, 21.0), ("clusters", 150, 8, 31, 10.0), ("clusters", 131, 6, 16, 5.0),
             ("gaussian", 5, 3, 4, 1.5), ("duplicates", 91, 5, 16, 5.0)]


def _case(kind, N, dim, k, seed=11):
    if kind == "gaussian":
        X, cluster = R.gaussian(seed, N, dim), None
    elif kind == "clusters":
        X, cluster = R.clusters(seed, N, dim)
    else:
        X, cluster = R.duplicates(seed, N, dim, group=7), None
    rng = np.random.default_rng(seed + 1)
    idx, dist = R.cosine_knn(X, k)
    label = (cluster if cluster is not None else rng.integers(0, 3, N)).astype(np.int32)
    label[rng.random(N) < 0.1] = -1
    batch = rng.integers(0, 2, N).astype(np.int32)
    batch[rng.random(N) < 0.05] = -1
    return idx, dist, batch, label


def _close(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool((both_nan | (np.abs(got - want) <= tol * np.abs(want))).all())


@pytest.mark.parametrize("kind, N, dim, k, perplexity", CPU_CASES)
def test_cpu_plumbing_path_equals_the_restatement(kind, N, dim, k, perplexity):
    from mmvae_amd import backend, mixing

    idx, dist, batch, label = _case(kind, N, dim, k)
    rbeta, rtries, firm = R.calibrate(dist, perplexity)
    assert firm.mean() >= 0.99
    t = torch.from_numpy
    with backend.cpu_plumbing():
        beta, tries = mixing.calibrate(t(idx), t(dist), perplexity)
        assert beta.dtype == torch.float64 and tries.dtype == torch.int32
        assert np.array_equal(beta.numpy()[firm], rbeta[firm]) and np.array_equal(tries.numpy()[firm], rtries[firm])
        codes = np.stack([batch, label])
        got = mixing.lisi(t(idx), t(dist), t(codes), beta=t(rbeta))
        assert got.shape == (2, N)
        for c in range(2):
            assert _close(got[c].numpy(), R.lisi(idx, dist, rbeta, codes[c]), 1e-12), c
        one = mixing.lisi(t(idx), t(dist), t(label), perplexity)  # a single column, calibrated inside
        assert one.shape == (N,) and _close(one.numpy()[firm], got[1].numpy()[firm], 1e-12)
        pred, conf, cross = mixing.label_transfer(t(idx), t(dist), t(batch), t(label), beta=t(rbeta))
    rpred, rconf, rcross, margin = R.transfer(idx, dist, rbeta, batch, label)
    sure = margin > 1e-9
    assert pred.dtype == torch.int32 and np.array_equal(pred.numpy()[sure], rpred[sure])
    assert np.array_equal(pred.numpy() < 0, rpred < 0)
    assert _close(conf.numpy()[sure], rconf[sure], 1e-12) and _close(cross.numpy(), rcross, 1e-12)
    if kind == "duplicates":  # runs of 7 equal rows: 6 neighbours at distance 0, more than the perplexity -- H never falls to log 5
        assert (rtries == R.MAX_TRIES).all() and (rbeta == 2.0 ** 50).all()


def test_default_perplexity_is_a_third_of_the_neighbours():
    from mmvae_amd import backend, mixing

    assert mixing.default_perplexity(64) == 21.0
    idx, dist, _, label = _case("gaussian", 40, 5, 16)
    with backend.cpu_plumbing():
        a = mixing.calibrate(torch.from_numpy(idx), torch.from_numpy(dist))
        b = mixing.calibrate(torch.from_numpy(idx), torch.from_numpy(dist), 5.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cpu_tensors_are_refused_outside_cpu_plumbing():
    from mmvae_amd import mixing

    idx, dist, batch, label = (torch.from_numpy(a) for a in _case("gaussian", 20, 4, 6))
    beta = torch.ones(20, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        mixing.calibrate(idx, dist, 2.0)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        mixing.lisi(idx, dist, label, beta=beta)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        mixing.label_transfer(idx, dist, batch, label, beta=beta)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        mixing.integration_metrics(torch.rand(20, 4), pd.DataFrame({"species": ["a"] * 20, "cell_type": ["b"] * 20}),
                                   n_neighbors=6)


def test_arguments_are_validated():
    from mmvae_amd import backend, mixing

    idx, dist, batch, label = (torch.from_numpy(a) for a in _case("gaussian", 20, 4, 6))
    beta = torch.ones(20, dtype=torch.float64)
    with backend.cpu_plumbing():
        for u in (1.0, 5.0, 0.5, float("nan")):
            with pytest.raises(ValueError, match="perplexity"):
                mixing.calibrate(idx, dist, u)
        with pytest.raises(ValueError, match="perplexity"):
            mixing.calibrate(idx[:, :4], dist[:, :4])  # the default (k - 1) / 3 = 1 is no perplexity at k = 4
        with pytest.raises(ValueError, match="k <= 64"):
            mixing.calibrate(idx[:, :2], dist[:, :2], 1.5)
        with pytest.raises(ValueError, match="k <= 64"):
            mixing.calibrate(torch.zeros((3, 65), dtype=torch.int32), torch.zeros((3, 65)), 21.0)
        with pytest.raises(ValueError, match=r"\[N, k\]"):
            mixing.calibrate(idx, dist[:, :5], 2.0)
        with pytest.raises(TypeError, match="int32"):
            mixing.calibrate(idx.long(), dist, 2.0)
        with pytest.raises(TypeError, match="int32"):
            mixing.lisi(idx, dist, label.long(), beta=beta)
        with pytest.raises(ValueError, match="codes must be"):
            mixing.lisi(idx, dist, label[:19], beta=beta)
        with pytest.raises(ValueError, match="not both"):
            mixing.lisi(idx, dist, label, 2.0, beta)
        with pytest.raises(TypeError, match="float64"):
            mixing.lisi(idx, dist, label, beta=beta.float())
        with pytest.raises(ValueError, match="must be \\[N\\]"):
            mixing.label_transfer(idx, dist, torch.stack([batch, batch]), label, beta=beta)
        wild = idx.clone()
        wild[3, 2] = 20
        with pytest.raises(ValueError, match="neighbour indices"):
            mixing.lisi(wild, dist, label, beta=beta)
        wild[3, 2] = -1
        with pytest.raises(ValueError, match="neighbour indices"):
            mixing.label_transfer(wild, dist, batch, label, beta=beta)
        with pytest.raises(KeyError, match="tissue"):
            mixing.integration_metrics(torch.rand(20, 4), pd.DataFrame({"species": ["a"] * 20}), label_keys=("tissue",),
                                       n_neighbors=6)
        with pytest.raises(ValueError, match="metadata rows"):
            mixing.integration_metrics(torch.rand(20, 4), pd.DataFrame({"species": ["a"] * 19, "cell_type": ["b"] * 19}),
                                       n_neighbors=6)


def test_summary_tables_on_a_hand_made_case():
    from mmvae_amd import mixing

    nan = float("nan")
    values = torch.tensor([[1.0, 2.0, 2.0, nan, 1.5], [1.0, 1.0, 3.0, 1.0, 1.0]])
    table = mixing.summarise_lisi(values, ["species", "cell_type"], ["batch", "label"], [2, 5])
    assert tuple(table.columns) == mixing.SUMMARY_COLUMNS
    assert table["column"].tolist() == ["species", "cell_type"] and table["role"].tolist() == ["batch", "label"]
    assert table["n_classes"].tolist() == [2, 5] and table["n_cells"].tolist() == [4, 5]
    assert table["mean_lisi"].tolist() == [1.625, 1.4]
    assert table["median_lisi"].tolist() == [1.5, 1.0]  # (torch's median of an even count: the lower middle value)
    assert table["scaled_lisi"].tolist() == [0.5, 0.0]
    one = mixing.summarise_lisi(values[:1], ["species"], ["batch"], [1])
    assert math.isnan(one["scaled_lisi"][0])

    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    batch = i32(0, 0, 0, 1, 1, 1, -1, 1)
    label = i32(0, 1, -1, 0, 1, 1, 0, 2)
    pred = i32(0, 0, 1, 0, -1, 1, 0, 1)
    cross = torch.tensor([0.5, 0.25, 0.75, 1.0, 0.0, 0.5, 0.25, 0.5])
    rows, confusion = mixing.summarise_transfer("cell_type", batch, label, pred, cross, ["human", "mouse"], ["T", "B", "NK"])
    table = pd.DataFrame(rows, columns=list(mixing.TRANSFER_COLUMNS))
    assert table["label"].tolist() == ["cell_type"] * 3 and table["batch"].tolist() == ["human", "mouse", "all"]
    assert table["n_cells"].tolist() == [3, 4, 8] and table["n_scored"].tolist() == [2, 3, 6]
    assert table["accuracy"].tolist() == [0.5, 2 / 3, 4 / 6]
    assert table["mean_cross"].tolist() == [0.5, 0.5, 3.75 / 8]
    assert table["share_without_neighbour"].tolist() == [0.0, 0.25, 0.125]
    assert confusion.index.tolist() == ["T", "B", "NK"] == confusion.columns.tolist()
    assert confusion.values.tolist() == [[3, 0, 0], [1, 1, 0], [0, 1, 0]]


def _frame(n, species, cell_type):
    return pd.DataFrame({"species": species, "cell_type": cell_type, "cell": [f"c{i}" for i in range(n)]})


def test_integration_metrics_on_cpu_plumbing():
    from mmvae_amd import backend, mixing

    X, cluster = R.clusters(5, 60, 6, n_clusters=2, spread=0.05)
    species = np.where(np.arange(60) % 2 == 0, "human", "mouse").astype(object)
    cell_type = np.where(cluster == 0, "T", "B").astype(object)
    cell_type[7] = np.nan
    with backend.cpu_plumbing():
        out = mixing.integration_metrics(torch.from_numpy(X), _frame(60, species, cell_type), n_neighbors=10)
        lonely = mixing.integration_metrics(torch.from_numpy(X), _frame(60, species, cell_type), n_neighbors=10,
                                            transfer=False)
    assert out.columns == ("species", "cell_type") and out.idx.shape == (60, 10) and out.lisi.shape == (2, 60)
    assert list(out.categories["species"]) == ["human", "mouse"] and list(out.categories["cell_type"]) == ["B", "T"]
    assert out.codes[1, 7] == -1 and out.codes.dtype == torch.int32
    assert tuple(out.summary.columns) == mixing.SUMMARY_COLUMNS and out.summary["n_classes"].tolist() == [2, 2]
    # the species alternate inside the clusters and the clusters are far apart: mixed batches (about three effective
    # neighbours of two even classes: 1 / (1/2 + 1/6) = 1.5 expected, far from the 1.0 of unmixed ones), pure labels
    assert out.summary["median_lisi"][0] > 1.2 and out.summary["median_lisi"][1] == 1.0
    assert out.summary["scaled_lisi"][1] == 0.0
    want = R.lisi(out.idx.numpy(), out.dist.numpy().astype(np.float32), out.beta.numpy(), out.codes[0].numpy())
    assert np.abs(out.lisi[0].numpy() - want).max() <= 1e-6  # (the restatement reads the distances rounded to fp32)
    assert tuple(out.transfer_summary.columns) == mixing.TRANSFER_COLUMNS
    assert out.transfer_summary["batch"].tolist() == ["human", "mouse", "all"]
    assert out.transfer_summary["accuracy"].tolist() == [1.0, 1.0, 1.0]
    assert out.transfer_summary["n_scored"].tolist()[2] == 59 and out.transfer_summary["n_cells"].tolist() == [30, 30, 60]
    assert int(out.confusion["cell_type"].values.sum()) == 59 and int(np.trace(out.confusion["cell_type"].values)) == 59
    assert int(out.pred["cell_type"][7]) == out.categories["cell_type"].get_loc("T" if cluster[7] == 0 else "B")
    assert lonely.transfer_summary is None and not lonely.pred and torch.equal(lonely.lisi, out.lisi)


def _tool():
    spec = importlib.util.spec_from_file_location("integration_metrics_tool",
                                                  os.path.join(ROOT, "tools", "integration_metrics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_end_to_end_on_a_directory_and_an_h5(tmp_path, monkeypatch, capsys):
    from mmvae_amd import backend
    from mmvae_amd import predictions as P

    tool = _tool()
    monkeypatch.delenv("DIRECTORY", raising=False)
    X, cluster = R.clusters(9, 50, 5, n_clusters=2, spread=0.05)
    meta = _frame(50, np.where(np.arange(50) % 2 == 0, "human", "mouse"), np.where(cluster == 0, "T", "B"))
    meta["tissue"] = np.where(np.arange(50) < 25, "lung", "gut")
    np.savez(tmp_path / "z_embeddings.npz", embeddings=X.astype(np.float32))
    meta.to_pickle(tmp_path / "z_metadata.pkl")
    a = tool.parse_args(["--directory", str(tmp_path), "--keys", "z", "--labels", "cell_type", "--labels", "tissue"])
    assert (a.batch, a.labels, a.keys, a.save_dir, a.n_neighbors, a.perplexity) == \
        ("species", ["cell_type", "tissue"], ["z"], None, 64, None)
    assert tool.parse_args(["--directory", str(tmp_path), "--keys", "z"]).labels == ["cell_type"]
    with pytest.raises(SystemExit):
        tool.parse_args(["--directory", str(tmp_path / "absent"), "--keys", "z"])
    out_dir = tmp_path / "tables"
    with backend.cpu_plumbing():
        assert tool.main(["--directory", str(tmp_path), "--keys", "z", "--batch", "species", "--labels", "cell_type",
                          "--labels", "tissue", "--n_neighbors", "10", "--save_dir", str(out_dir)]) == 0
    printed = capsys.readouterr().out.split()
    names = ["integration_metrics.z.csv", "integration_metrics.z.transfer.csv",
             "integration_metrics.z.confusion.cell_type.csv", "integration_metrics.z.confusion.tissue.csv"]
    assert printed == [str(out_dir / n) for n in names] and all(os.path.exists(p) for p in printed)
    table = pd.read_csv(out_dir / names[0])
    assert table["column"].tolist() == ["species", "cell_type", "tissue"] and table["median_lisi"][1] == 1.0
    assert pd.read_csv(out_dir / names[1])["accuracy"].tolist()[:3] == [1.0, 1.0, 1.0]
    # the predictions.h5 form, LISI only: the same numbers next to the file
    h5 = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(X.astype(np.float32), meta, h5, "z")
    with backend.cpu_plumbing():
        assert tool.main(["--directory", h5, "--keys", "z", "--labels", "cell_type", "--labels", "tissue",
                          "--n_neighbors", "10", "--no-transfer"]) == 0
    assert capsys.readouterr().out.split() == [str(tmp_path / names[0])]
    again = pd.read_csv(tmp_path / names[0])
    assert np.allclose(again["median_lisi"], table["median_lisi"], rtol=0, atol=1e-12)


def test_trainer_integration_metrics_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend, mixing
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
        k = min(8, 2 * B - 1)
        assert k >= 5
        batches = [(x, pd.DataFrame({"group": ["a"] * B, "donor": [f"d{i % 2}" for i in range(B)]}), eid),
                   (x.flip(0) * 0.5, pd.DataFrame({"group": ["b"] * B, "donor": [f"d{i % 2}" for i in range(B)]}), eid)]
        out = Trainer().integration_metrics(model, batches, batch_key="donor", label_keys=("group", "species"),
                                            n_neighbors=k)
    assert isinstance(out, mixing.IntegrationMetrics) and out.columns == ("donor", "group", "species")
    assert out.idx.shape == (2 * B, k) and out.lisi.shape == (3, 2 * B) and out.codes.shape == (3, 2 * B)
    assert list(out.categories["species"]) == [eid] and bool(((out.lisi[2] - 1.0).abs() <= 1e-12).all())  # one class
    assert out.summary["n_classes"].tolist() == [2, 2, 1] and math.isnan(out.summary["scaled_lisi"][2])
    assert set(out.pred) == {"group", "species"} and out.transfer_summary["label"].tolist() == ["group"] * 3 + ["species"] * 3
