"""Host-side checks of the silhouette widths (no GPU): the C-ABI surface of libmmvae_sil.so and its argument checks,
`sort_runs` on hand-made codes, the fp64 CPU-plumbing path of mmvae_amd.silhouette against the independent restatement
(tests/sil_restatement.py), the restatement itself against scikit-learn where that is installed, and the tables, the
Trainer method and the command-line tool end to end on a temporary directory."""
import importlib.util
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import sil_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_sil.h")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _bind, _sil_lib

    declared = check_surface(_sil_lib.BINDING)
    assert set(declared) == {"mmvae_sil_abi_version", "mmvae_sil_build_arch", "mmvae_sil_rows_workspace_bytes",
                             "mmvae_sil_rows_f32"} == set(_sil_lib.SIL_PROTOTYPES)
    assert "_sil_lib" in _bind.DEVICE_LIBRARY_MODULES and len(_bind.DEVICE_LIBRARY_MODULES) == 10


def test_versions_and_constants():
    from mmvae_amd import _lib, _mix_lib, _sil_lib, _umap_lib, silhouette

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _sil_lib.load_sil()
    assert define("MMVAE_SIL_ABI_VERSION") == 1 == lib.mmvae_sil_abi_version() == _sil_lib.SIL_ABI_VERSION
    assert lib.mmvae_sil_build_arch() == b"gfx950"
    assert define("MMVAE_SIL_MAX_D") == _sil_lib.SIL_MAX_D == silhouette.MAX_D == 512
    assert define("MMVAE_SIL_EUCLIDEAN") == _sil_lib.SIL_EUCLIDEAN == silhouette.METRICS["euclidean"] == 0
    assert define("MMVAE_SIL_COSINE") == _sil_lib.SIL_COSINE == silhouette.METRICS["cosine"] == 1
    # the training library, the UMAP library and the mixing library are untouched: same versions, none of the new names
    assert _lib.load().mmvae_abi_version() == 16 and _umap_lib.load_umap().mmvae_umap_abi_version() == 1
    assert _mix_lib.load_mix().mmvae_mix_abi_version() == 1
    others = list(_lib.PROTOTYPES) + list(_umap_lib.UMAP_PROTOTYPES) + list(_mix_lib.MIX_PROTOTYPES)
    assert not [n for n in others if n.startswith("mmvae_sil_")]


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below carries the fake device address 16: had one of them launched, it would not return ERR_ARG."""
    from mmvae_amd import _sil_lib

    lib = _sil_lib.load_sil()
    size = lib.mmvae_sil_rows_workspace_bytes
    N, D = 100, 70
    need = size(N, D)
    assert need == 128 * 128 * 4 + 128 * 4 + 128 * 4  # 128 padded rows of 128 columns, their norms, their runs
    assert size(1, 1) == 64 * 64 * 4 + 64 * 8 and size(64, 512) == 64 * 512 * 4 + 64 * 8 and size(65, 65) % 16 == 0
    for shape in ((0, 8), (-1, 8), (10, 0), (10, -2), (10, 513)):
        assert size(*shape) == 0, shape
    for n in (1, 5, 64, 1000, 100000):
        for d in (1, 64, 65, 128, 129, 512):
            assert size(n, d) > 0 and size(n, d) % 16 == 0 and size(n, d) <= 4 * (n + 63) * (max(2 * d, 64) + 2)
    #     N  D  x  ldx metric R run_ptr run_group a  b  nearest s  workspace bytes stream
    ok = (N, D, 16, D, 0, 3, 16, 16, 16, 16, 16, 16, 16, need, None)
    bad = {"N 0": {0: 0}, "N < 0": {0: -3}, "D 0": {1: 0, 3: 0}, "D 513": {1: 513, 3: 513}, "ldx < D": {3: D - 1},
           "R 0": {5: 0}, "R > N": {5: N + 1}, "metric 2": {4: 2}, "metric -1": {4: -1}, "short workspace": {13: need - 1},
           "no workspace": {13: 0}, "misaligned workspace": {12: 24}}
    bad.update({f"null argument {i}": {i: None} for i in (2, 6, 7, 8, 9, 10, 11, 12)})
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_sil_rows_f32(*args) == _sil_lib.ERR_ARG, what


def test_sort_runs_on_hand_made_codes():
    from mmvae_amd.silhouette import sort_runs

    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    cls = i32(2, 0, -1, 2, 0, 1, 0, 2, 1)
    group = i32(1, 0, 0, 0, 1, -1, 0, 1, 0)
    order, run_ptr, run_group, run_class = sort_runs(cls, group)
    # group 0: class 0 -> cells 1, 6; class 1 -> 8; class 2 -> 3.  group 1: class 0 -> 4; class 2 -> 0, 7 (stable)
    assert order.tolist() == [1, 6, 8, 3, 4, 0, 7] and order.dtype == torch.int64
    assert run_ptr.tolist() == [0, 2, 3, 4, 5, 7] and run_ptr.dtype == torch.int32
    assert run_group.tolist() == [0, 0, 0, 1, 1] and run_class.tolist() == [0, 1, 2, 0, 2]
    assert run_group.dtype == torch.int32 and run_class.dtype == torch.int32
    want = R.sorted_runs(cls.numpy(), group.numpy())
    assert all(np.array_equal(g.numpy(), w) for g, w in zip((order, run_ptr, run_group, run_class), want))
    # a single group: negative classes dropped, the others in class order, the original order kept inside a class
    order, run_ptr, run_group, run_class = sort_runs(cls)
    assert order.tolist() == [1, 4, 6, 5, 8, 0, 3, 7] and run_ptr.tolist() == [0, 3, 5, 8]
    assert run_group.tolist() == [0, 0, 0] and run_class.tolist() == [0, 1, 2]
    # every cell its own class (codes need not be dense), int64 codes
    order, run_ptr, run_group, run_class = sort_runs(torch.tensor([7, 3, 900, 5]))
    assert order.tolist() == [1, 3, 0, 2] and run_ptr.tolist() == [0, 1, 2, 3, 4] and run_class.tolist() == [3, 5, 7, 900]
    # nothing kept
    order, run_ptr, run_group, run_class = sort_runs(i32(-1, -1))
    assert order.numel() == 0 and run_ptr.tolist() == [0] and run_group.numel() == 0 and run_class.numel() == 0
    with pytest.raises(ValueError, match=r"\[N\]"):
        sort_runs(cls, group[:3])


def _case(N, D, C, G, seed=5, unlabelled=True):
    X, cls = R.clusters(seed, N, D, C)
    rng = np.random.default_rng(seed + 1)
    group = rng.integers(0, G, N).astype(np.int32)
    if unlabelled:
        cls[rng.random(N) < 0.1] = -1
        group[rng.random(N) < 0.05] = -1
    cls[0], group[0] = C, 0          # a class of one cell
    group[1:3], cls[1:3] = G, 0      # a group of one class
    return X, cls, group


def _agree(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and (np.abs(got - want)[~np.isnan(want)] <= tol).all())


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("N, D, C, G", [(5, 3, 2, 1), (70, 8, 3, 1), (150, 20, 4, 3)])
def test_cpu_plumbing_path_equals_the_restatement(N, D, C, G, metric):
    from mmvae_amd import backend, silhouette

    X, cls, group = _case(N, D, C, G, unlabelled=N > 5)
    if metric == "euclidean":
        X = R.with_duplicates(X, cls, 1)
    a, b, s, nearest, lead = R.silhouette(X, cls, group, metric)
    t = torch.from_numpy
    with backend.cpu_plumbing():
        got = silhouette.silhouette_samples(t(X), t(cls), t(group), metric)
        flat = silhouette.silhouette_samples(t(X), t(cls), None, metric)
    assert isinstance(got, silhouette.SilhouetteRows) and got.a.dtype == torch.float64 and got.nearest.dtype == torch.int32
    assert _agree(got.a, a, 1e-12) and _agree(got.b, b, 1e-12) and _agree(got.s, s, 1e-10)
    sure = lead > 1e-9
    assert np.array_equal(got.nearest.numpy()[sure], nearest[sure]) and np.array_equal(got.nearest.numpy() < 0, nearest < 0)
    assert got.a[0] == 0 and got.s[0] == 0
    assert np.isnan(got.b.numpy()[1:3]).all() and (got.nearest.numpy()[1:3] == -1).all()
    assert np.isnan(got.s.numpy()[1:3]).all() and (got.a.numpy()[1:3] >= 0).all()
    if metric == "euclidean":
        ones = (cls == 1) & (group >= 0)
        assert (got.a.numpy()[ones] == 0).all()  # copies of one row
    a1, b1, s1, _, _ = R.silhouette(X, cls, None, metric)
    assert _agree(flat.a, a1, 1e-12) and _agree(flat.b, b1, 1e-12) and _agree(flat.s, s1, 1e-10)


def test_cpu_tensors_are_refused_outside_cpu_plumbing_and_arguments_are_validated():
    from mmvae_amd import backend, silhouette

    X, cls, group = _case(20, 4, 2, 1)
    x, c, g = torch.from_numpy(X), torch.from_numpy(cls), torch.from_numpy(group)
    frame = pd.DataFrame({"species": ["a", "b"] * 10, "cell_type": ["x"] * 20})
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        silhouette.silhouette_samples(x, c, g)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        silhouette.silhouette_widths(x, frame)
    order, run_ptr, run_group, _ = silhouette.sort_runs(c, g)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        silhouette.silhouette_rows(x[order], run_ptr, run_group)
    with backend.cpu_plumbing():
        with pytest.raises(ValueError, match="metric"):
            silhouette.silhouette_samples(x, c, g, "manhattan")
        with pytest.raises(ValueError, match="codes must be"):
            silhouette.silhouette_samples(x, c[:19], g)
        with pytest.raises(TypeError, match="int32 or int64"):
            silhouette.silhouette_samples(x, c.float(), g)
        with pytest.raises(ValueError, match="D <= 512"):
            silhouette.silhouette_samples(torch.zeros(20, 513), c)
        with pytest.raises(KeyError, match="tissue"):
            silhouette.silhouette_widths(x, frame, label_keys=("tissue",))
        with pytest.raises(ValueError, match="metadata rows"):
            silhouette.silhouette_widths(x, frame[:19])
        nothing = silhouette.silhouette_samples(x, torch.full_like(c, -1))
    assert bool(torch.isnan(nothing.s).all() and (nothing.nearest == -1).all())


def test_restatement_equals_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    N, D = 300, 12
    X, label = R.clusters(3, N, D, 5)
    rng = np.random.default_rng(4)
    batch = rng.integers(0, 3, N).astype(np.int32)
    for metric in ("euclidean", "cosine"):
        a, b, s, _, _ = R.silhouette(X, label, None, metric)
        want = metrics.silhouette_samples(X, label, metric=metric)
        assert np.abs(s - want).max() <= 2e-8, metric
        # with groups: scikit-learn on each label's subset
        _, _, sg, _, _ = R.silhouette(X, batch, label, metric)
        for c in np.unique(label):
            sub = label == c
            assert np.abs(sg[sub] - metrics.silhouette_samples(X[sub], batch[sub], metric=metric)).max() <= 2e-8, (metric, c)
    # scIB's silhouette_batch written out: per label 1 - |s| on the subset, labels with one batch or only singletons skipped
    _, _, sg, _, _ = R.silhouette(X, batch, label)
    per = []
    for c in np.unique(label):
        sub = label == c
        n_batches = len(np.unique(batch[sub]))
        if n_batches == 1 or n_batches == sub.sum():
            continue
        per.append(np.mean(1 - np.abs(metrics.silhouette_samples(X[sub], batch[sub]))))
    from mmvae_amd import silhouette

    t = torch.from_numpy
    assert abs(R.asw_batch(sg, label, batch) - np.mean(per)) <= 2e-8
    assert abs(silhouette.asw_batch(t(sg), t(label), t(batch)) - np.mean(per)) <= 2e-8
    assert abs(silhouette.asw_label(t(s)) - metrics.silhouette_score(X, label, metric="cosine")) <= 2e-8


def test_averages_on_hand_made_values():
    from mmvae_amd import silhouette

    nan = float("nan")
    s = torch.tensor([0.5, -0.25, nan, 1.0, 0.0, 0.0, nan, -0.5], dtype=torch.float64)
    assert silhouette.asw_label(s) == (0.5 - 0.25 + 1.0 - 0.5) / 6 and silhouette.asw_label(s, scaled=True) == (0.125 + 1) / 2
    assert math.isnan(silhouette.asw_label(torch.tensor([nan])))
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    label = i32(0, 0, 1, 2, 3, 3, 1, 0)
    batch = i32(0, 1, 0, 0, 0, 1, 0, 1)
    # label 0: (0.5 + 0.75 + 0.5) / 3; label 1: no defined s; label 2: 1 - 1 = 0; label 3: two cells, two batches, 1 - 0 = 1
    assert silhouette.asw_batch(s, label) == (1.75 / 3 + 0.0 + 1.0) / 3
    assert silhouette.asw_batch(s, label, batch) == 1.75 / 3     # labels 2 and 3: every batch a single cell
    assert silhouette.asw_batch(s, torch.where(label == 0, -1, label)) == 0.5  # unlabelled cells belong to no label
    assert math.isnan(silhouette.asw_batch(s, i32(*[-1] * 8)))


def _frame(n, species, cell_type):
    return pd.DataFrame({"species": species, "cell_type": cell_type, "cell": [f"c{i}" for i in range(n)]})


def _two_batches(n=90, seed=9):
    X, cluster = R.clusters(seed, n, 6, 3, spread=0.1)
    species = np.where(np.arange(n) % 2 == 0, "human", "mouse").astype(object)
    cell_type = np.array(["B", "NK", "T"], dtype=object)[cluster]
    return X, cluster, species, cell_type


def test_silhouette_widths_on_cpu_plumbing():
    from mmvae_amd import backend, silhouette

    X, cluster, species, cell_type = _two_batches()
    cell_type[7] = np.nan
    with backend.cpu_plumbing():
        out = silhouette.silhouette_widths(torch.from_numpy(X), _frame(90, species, cell_type))
        cosine = silhouette.silhouette_widths(torch.from_numpy(X), _frame(90, species, cell_type), metric="cosine")
    assert out.columns == ("species", "cell_type") and out.codes.shape == (2, 90) and out.codes.dtype == torch.int32
    assert list(out.categories["species"]) == ["human", "mouse"] and list(out.categories["cell_type"]) == ["B", "NK", "T"]
    batch, label = out.codes[0].numpy(), out.codes[1].numpy()
    assert label[7] == -1 and np.array_equal(np.delete(label, 7), np.delete(cluster, 7))
    _, _, s_label, near, _ = R.silhouette(X, label, None)
    _, _, s_batch, _, _ = R.silhouette(X, batch, label)
    assert _agree(out.label_rows["cell_type"].s, s_label, 1e-10) and _agree(out.batch_rows["cell_type"].s, s_batch, 1e-10)
    assert np.array_equal(out.label_rows["cell_type"].nearest.numpy(), near)
    assert tuple(out.summary.columns) == silhouette.SUMMARY_COLUMNS
    assert out.summary["column"].tolist() == ["cell_type", "cell_type"] and out.summary["role"].tolist() == ["label", "batch"]
    assert out.summary["n_classes"].tolist() == [3, 3] and out.summary["n_cells"].tolist() == [89, 89]
    assert abs(out.summary["asw"][0] - R.asw_label(s_label)) <= 1e-10
    assert abs(out.summary["asw"][1] - R.asw_batch(s_batch, label, batch)) <= 1e-10
    assert out.summary["scaled"].tolist() == [(out.summary["asw"][0] + 1) / 2, out.summary["asw"][1]]
    assert out.summary["asw"][0] > 0.8 and out.summary["asw"][1] > 0.9   # tight clusters, the species alternating in them
    table = out.per_label["cell_type"]
    assert tuple(table.columns) == silhouette.PER_LABEL_COLUMNS and table.index.tolist() == ["B", "NK", "T"]
    frame = pd.DataFrame({"label": label, "batch": batch, "s": s_label, "w": 1 - np.abs(s_batch)})[label >= 0]
    by = frame.groupby("label")
    assert table["n_cells"].tolist() == by.size().tolist() and table["n_batches"].tolist() == [2, 2, 2]
    assert np.abs(table["label_asw"].values - by["s"].mean().values).max() <= 1e-10
    assert np.abs(table["batch_asw"].values - by["w"].mean().values).max() <= 1e-10
    assert cosine.metric == "cosine" and cosine.summary["asw"][0] != out.summary["asw"][0]


def test_batch_asw_sees_batches_that_form_separate_blobs():
    """Two cell types; in the first the species are mixed, in the second they sit in two blobs of their own: the batch
    ASW of the second falls, whatever the local picture."""
    from mmvae_amd import backend, silhouette

    rng = np.random.default_rng(2)
    n = 80
    species = np.where(np.arange(n) % 2 == 0, "human", "mouse").astype(object)
    cell_type = np.where(np.arange(n) < 40, "mixed", "split").astype(object)
    X = 0.05 * rng.standard_normal((n, 4))
    X[40:, 0] += 5.0
    X[40:, 1] += np.where(np.arange(40) % 2 == 0, 1.0, -1.0)
    with backend.cpu_plumbing():
        out = silhouette.silhouette_widths(torch.from_numpy(X), _frame(n, species, cell_type))
    table = out.per_label["cell_type"]
    assert table.index.tolist() == ["mixed", "split"]
    assert table["batch_asw"]["mixed"] > 0.8 and table["batch_asw"]["split"] < 0.1
    assert abs(out.summary["asw"][1] - table["batch_asw"].mean()) <= 1e-12


def _tool():
    spec = importlib.util.spec_from_file_location("silhouette_widths_tool", os.path.join(ROOT, "tools", "silhouette_widths.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_end_to_end_on_a_directory_and_an_h5(tmp_path, monkeypatch, capsys):
    from mmvae_amd import backend, silhouette
    from mmvae_amd import predictions as P

    tool = _tool()
    monkeypatch.delenv("DIRECTORY", raising=False)
    X, cluster, species, cell_type = _two_batches(60)
    meta = _frame(60, species, cell_type)
    meta["tissue"] = np.where(np.arange(60) < 30, "lung", "gut")
    np.savez(tmp_path / "z_embeddings.npz", embeddings=X.astype(np.float32))
    meta.to_pickle(tmp_path / "z_metadata.pkl")
    a = tool.parse_args(["--directory", str(tmp_path), "--keys", "z", "--labels", "cell_type", "--labels", "tissue"])
    assert (a.batch, a.labels, a.keys, a.save_dir, a.metric) == ("species", ["cell_type", "tissue"], ["z"], None, "euclidean")
    assert tool.parse_args(["--directory", str(tmp_path), "--keys", "z"]).labels == ["cell_type"]
    with pytest.raises(SystemExit):
        tool.parse_args(["--directory", str(tmp_path / "absent"), "--keys", "z"])
    with pytest.raises(SystemExit):
        tool.parse_args(["--directory", str(tmp_path), "--keys", "z", "--metric", "manhattan"])
    out_dir = tmp_path / "tables"
    with backend.cpu_plumbing():
        assert tool.main(["--directory", str(tmp_path), "--keys", "z", "--batch", "species", "--labels", "cell_type",
                          "--labels", "tissue", "--save_dir", str(out_dir)]) == 0
        direct = silhouette.silhouette_widths(torch.from_numpy(X.astype(np.float32)), meta, "species", ("cell_type", "tissue"))
    printed = capsys.readouterr().out.split()
    names = ["silhouette.z.csv", "silhouette.z.cell_type.csv", "silhouette.z.tissue.csv"]
    assert printed == [str(out_dir / n) for n in names] and all(os.path.exists(p) for p in printed)
    table = pd.read_csv(out_dir / names[0])
    assert table["column"].tolist() == ["cell_type", "cell_type", "tissue", "tissue"]
    assert table["role"].tolist() == ["label", "batch"] * 2
    assert np.allclose(table["asw"], direct.summary["asw"], rtol=0, atol=1e-12) and table["asw"][0] > 0.8
    per = pd.read_csv(out_dir / names[1], index_col=0)
    assert per.index.tolist() == ["B", "NK", "T"] and tuple(per.columns) == silhouette.PER_LABEL_COLUMNS
    # the predictions.h5 form, cosine: the tables next to the file
    h5 = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(X.astype(np.float32), meta, h5, "z")
    with backend.cpu_plumbing():
        assert tool.main(["--directory", h5, "--keys", "z", "--metric", "cosine"]) == 0
        with pytest.raises(KeyError):
            silhouette.widths_from_predictions(h5, ("absent",))
    assert capsys.readouterr().out.split() == [str(tmp_path / names[0]), str(tmp_path / names[1])]
    again = pd.read_csv(tmp_path / names[0])
    assert again["role"].tolist() == ["label", "batch"] and not np.allclose(again["asw"], table["asw"][:2])


def test_trainer_silhouette_widths_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend, silhouette
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
        batches = [(x, pd.DataFrame({"group": ["a"] * B, "donor": [f"d{i % 2}" for i in range(B)]}), eid),
                   (x.flip(0) * 0.5, pd.DataFrame({"group": ["b"] * B, "donor": [f"d{i % 2}" for i in range(B)]}), eid)]
        out = Trainer().silhouette_widths(model, batches, batch_key="donor", label_keys=("group", "species"))
        with pytest.raises(ValueError, match="no batches"):
            Trainer().silhouette_widths(model, [])
    assert isinstance(out, silhouette.SilhouetteWidths) and out.columns == ("donor", "group", "species")
    assert out.codes.shape == (3, 2 * B) and set(out.label_rows) == {"group", "species"} == set(out.batch_rows)
    assert out.label_rows["group"].s.shape == (2 * B,) and bool(torch.isfinite(out.label_rows["group"].s).all())
    assert list(out.categories["species"]) == [eid] and bool(torch.isnan(out.label_rows["species"].s).all())  # one class
    assert out.summary["column"].tolist() == ["group", "group", "species", "species"]
    assert out.summary["n_classes"].tolist()[:3] == [2, 2, 1] and math.isnan(out.summary["asw"][2])
    assert out.per_label["species"]["n_cells"].tolist() == [2 * B] and out.per_label["group"]["n_batches"].tolist() == [2, 2]
