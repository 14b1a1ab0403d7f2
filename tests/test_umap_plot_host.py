"""Host-side checks of the UMAP plots (no GPU): the C-ABI surface of libmmvae_plot.so and its argument checks, the numpy
path of mmvae_amd.plots.rasterize against an independent restatement (tests/plot_restatement.py), the label selection,
the view fit, the PNG writer, generate_umap's two input forms and the command-line tool's arguments."""
import itertools
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import plot_restatement as R
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_plot.h")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _plot_lib

    declared = check_surface(_plot_lib.BINDING)
    assert set(declared) == {"mmvae_plot_abi_version", "mmvae_plot_build_arch", "mmvae_plot_count_f32",
                             "mmvae_plot_composite_u8"} == set(_plot_lib.PLOT_PROTOTYPES)


def test_versions_and_constants():
    from mmvae_amd import _lib, _plot_lib

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _plot_lib.load_plot()
    assert define("MMVAE_PLOT_ABI_VERSION") == 1 == lib.mmvae_plot_abi_version() == _plot_lib.PLOT_ABI_VERSION
    assert lib.mmvae_plot_build_arch() == b"gfx950"
    assert define("MMVAE_PLOT_MAX_CLASSES") == _plot_lib.PLOT_MAX_CLASSES >= 16
    assert define("MMVAE_PLOT_MAX_MARKER") == _plot_lib.PLOT_MAX_MARKER == 8
    assert define("MMVAE_PLOT_MAX_SIDE") == _plot_lib.PLOT_MAX_SIDE
    assert (define("MMVAE_PLOT_COUNT_DEFAULT"), define("MMVAE_PLOT_COUNT_PLAIN"), define("MMVAE_PLOT_COUNT_AGGREGATE")) \
        == (_plot_lib.PLOT_COUNT_DEFAULT, _plot_lib.PLOT_COUNT_PLAIN, _plot_lib.PLOT_COUNT_AGGREGATE)
    # the training library is untouched: same version, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_plot_")]


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below carries the fake device address 16: had one of them launched, it would not return ERR_ARG."""
    from mmvae_amd import _plot_lib

    lib = _plot_lib.load_plot()
    C = _plot_lib.PLOT_MAX_CLASSES
    view = _plot_lib.view_words([1, 0, 0, 0, 0, 1, 0, 0])
    #     n  dims pts ld codes classes W   H  m  view mode counts stream
    ok = (10, 2, 16, 2, 16, 15, 32, 32, 1, view, 0, 16, None)
    bad = {"n < 1": {0: 0}, "n < 0": {0: -5}, "dims 1": {1: 1, 3: 1}, "dims 4": {1: 4, 3: 4}, "classes 0": {5: 0},
           "classes max + 1": {5: C + 1}, "W 0": {6: 0}, "H 0": {7: 0}, "W -1": {6: -1}, "m 0": {8: 0}, "m 9": {8: 9},
           "ld < dims (2)": {3: 1}, "ld < dims (3)": {1: 3, 3: 2}, "mode 3": {10: 3}, "null points": {2: None},
           "null codes": {4: None}, "null view": {9: None}, "null counts": {11: None},
           "W too large": {6: _plot_lib.PLOT_MAX_SIDE + 1}}
    for what, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(ok)]
        assert lib.mmvae_plot_count_f32(*args) == _plot_lib.ERR_ARG, what
    #      counts classes W  H  colors alpha bg bg bg rgba stream
    okc = (16, 15, 32, 32, 16, 0.5, 1.0, 1.0, 1.0, 16, None)
    badc = {"alpha 0": {5: 0.0}, "alpha > 1": {5: 1.5}, "alpha nan": {5: float("nan")}, "alpha < 0": {5: -0.5},
            "classes 0": {1: 0}, "classes max + 1": {1: C + 1}, "W 0": {2: 0}, "H 0": {3: 0}, "null counts": {0: None},
            "null colors": {4: None}, "null rgba": {9: None}, "background 2": {7: 2.0}, "background -1": {6: -1.0},
            "misaligned rgba": {9: 18}}
    for what, change in badc.items():
        args = [change.get(i, a) for i, a in enumerate(okc)]
        assert lib.mmvae_plot_composite_u8(*args) == _plot_lib.ERR_ARG, what


# (N, W, H, classes, marker, dims)
CPU_CASES = [(1031, 37, 23, 15, 1, 2), (500, 37, 23, 16, 2, 3), (300, 16, 9, 3, 8, 2), (65, 1, 1, 1, 3, 2)]


@pytest.mark.parametrize("N, W, H, C, m, dims", CPU_CASES)
def test_cpu_plumbing_path_equals_the_restatement(N, W, H, C, m, dims):
    from mmvae_amd import backend, plots

    pts, codes = R.mixture(N, C, dims, seed=N)
    codes[::7] = -1
    codes[3::11] = C
    pts[5::13, 0] = np.nan
    colors = np.random.default_rng(1).uniform(0, 1, (C, 3)).astype(np.float32)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        plots.rasterize(torch.from_numpy(pts), codes, C, colors, W, H)
    with backend.cpu_plumbing():
        matrix = plots.view_matrix(30, 40) if dims == 3 else None
        # a view fitted to 80 % of the spread: markers get clipped at and fall off every border
        view = [w * s for w, s in zip(plots.fit_view(torch.from_numpy(pts), codes, W, H, matrix=matrix),
                                      (1.3, 1.3, 1.3, 1, 1.3, 1.3, 1.3, 1))]
        rgba, counts = plots.rasterize(torch.from_numpy(pts), codes, C, colors, W, H, view=view, marker_px=m, alpha=0.5,
                                       background=(1.0, 0.5, 0.0))
    want = R.count(pts, codes, C, W, H, m, view)
    assert counts.dtype == torch.int32 and rgba.dtype == torch.uint8 and tuple(rgba.shape) == (H, W, 4)
    assert np.array_equal(counts.numpy().view(np.uint32), want) and want.sum() > 0
    assert np.array_equal(rgba.numpy(), R.composite(want, colors, 0.5, (1.0, 0.5, 0.0)))


def test_closed_form_equals_the_mean_over_all_orders():
    """Section 2 of the header: the expectation over drawing orders has the closed form, for four points exhaustively."""
    rng = np.random.default_rng(0)
    class_colors = rng.uniform(0, 1, (3, 3))
    bg = (1.0, 0.9, 0.8)
    for alpha in (0.5, 0.25, 1.0, 0.9):
        for classes in itertools.product(range(3), repeat=4):
            want = R.mean_over_orders([class_colors[c] for c in classes], alpha, bg)
            counts = np.bincount(classes, minlength=3).reshape(3, 1, 1)
            got = R.composite_exact(counts, class_colors, alpha, bg)[0, 0] / 255.0
            # (class colours pass through float32 in the restatement: 2^-24 relative)
            assert np.abs(got - want).max() <= 1e-7, (alpha, classes)


def test_category_codes():
    from mmvae_amd.plots import category_codes

    col = ["b"] * 5 + ["a"] * 5 + ["c"] * 3 + [np.nan] * 2 + ["d"]
    md = pd.DataFrame({"k": col})
    chosen = md["k"].value_counts().nlargest(2).index  # a tie between a and b: pandas' own choice, whatever it is
    codes, labels = category_codes(md, "k", 2)
    assert codes.dtype == np.int32 and codes.shape == (16,) and labels == list(chosen) and set(labels) == {"a", "b"}
    for i, v in enumerate(col):
        assert codes[i] == (labels.index(v) if v in labels else -1)
    # fewer labels than n_largest
    codes, labels = category_codes(md, "k", 15)
    assert labels == list(md["k"].value_counts().nlargest(15).index) and len(labels) == 4
    assert (codes[13:15] == -1).all() and (codes[:13] >= 0).all() and codes[15] == labels.index("d")
    # bytes labels come back decoded; the rows are still found
    mdb = pd.DataFrame({"k": [b"x", b"y", b"x", b"z\xc3\xa9"]})
    codes, labels = category_codes(mdb, "k", 2)
    assert labels[0] == "x" and all(isinstance(v, str) for v in labels) and codes[0] == codes[2] == 0
    assert sorted(codes.tolist()) == [-1, 0, 0, 1]
    # a categorical column, with a category nobody has and a missing value
    cat = pd.Categorical(["u", "v", "u", None, "u"], categories=["v", "u", "w"])
    mdc = pd.DataFrame({"k": cat})
    codes, labels = category_codes(mdc, "k", 2)
    assert labels == ["u", "v"] and codes.tolist() == [0, 1, 0, -1, 0]
    with pytest.raises(ValueError, match="at most"):
        category_codes(pd.DataFrame({"k": np.arange(40)}), "k", 17)


def test_fit_view_margins_flip_and_dropped_rows():
    from mmvae_amd import backend, plots

    pts = np.array([[0.0, 10.0], [4.0, 30.0], [2.0, 20.0], [1000.0, -1000.0], [np.nan, 0.0], [np.inf, 5.0]], np.float32)
    codes = np.array([0, 1, 0, -1, 0, 1], np.int32)
    W, H = 220, 110
    with backend.cpu_plumbing():
        view = plots.fit_view(torch.from_numpy(pts), codes, W, H)
        # the limits are 5 % of the span beyond the plotted points: x -0.2 .. 4.2, y 9 .. 31; rows 3 .. 5 are ignored
        assert np.allclose(view, [50.0, 0, 0, 10.0, 0, -5.0, 0, 155.0], rtol=1e-12, atol=1e-12)
        u = lambda p: view[0] * p[0] + view[1] * p[1] + view[3]  # noqa: E731
        v = lambda p: view[4] * p[0] + view[5] * p[1] + view[7]  # noqa: E731
        assert np.isclose(u(pts[0]), 0.05 * W / 1.1) and np.isclose(u(pts[1]), W - 0.05 * W / 1.1)
        assert np.isclose(v(pts[1]), 0.05 * H / 1.1) and np.isclose(v(pts[0]), H - 0.05 * H / 1.1)  # y points up
        # a zero span is widened: all points on one vertical line
        line = np.array([[3.0, 1.0], [3.0, 2.0]], np.float32)
        lv = plots.fit_view(torch.from_numpy(line), [0, 0], W, H)
        assert np.isfinite(lv).all() and np.isclose(lv[0] * 3.0 + lv[3], W / 2)
        one = plots.fit_view(torch.from_numpy(line[:1]), [0], W, H)
        assert np.isfinite(one).all() and np.isclose(one[5] * 1.0 + one[7], H / 2)
        none = plots.fit_view(torch.from_numpy(line), [-1, -1], W, H)
        assert np.isfinite(none).all()
        # margin 0 and a 3-component embedding under a projection
        p3 = np.random.default_rng(0).standard_normal((50, 3)).astype(np.float32)
        M = plots.view_matrix(30, 75)
        v3 = plots.fit_view(torch.from_numpy(p3), np.zeros(50, np.int32), W, H, margin=0.0, matrix=M)
        uu = p3.astype(np.float64) @ np.array(v3[0:3]) + v3[3]
        vv = p3.astype(np.float64) @ np.array(v3[4:7]) + v3[7]
        assert np.isclose(uu.min(), 0) and np.isclose(uu.max(), W) and np.isclose(vv.min(), 0) and np.isclose(vv.max(), H)
    M = np.array(plots.view_matrix(30, 75))
    assert np.allclose(M @ M.T, np.eye(2), atol=1e-12)  # two orthonormal screen directions
    assert np.allclose(plots.view_matrix(90, 0), [[0, 1, 0], [-1, 0, 0]], atol=1e-12)  # seen from above


@pytest.mark.parametrize("W, H", [(1, 1), (37, 23), (1085, 616)])
def test_write_png_round_trip(tmp_path, W, H):
    from PIL import Image

    from mmvae_amd.plots import write_png

    img = np.random.default_rng(W).integers(0, 256, (H, W, 4), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    write_png(path, img)
    with Image.open(path) as im:
        assert im.mode == "RGBA" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), img)
    write_png(path, torch.from_numpy(img))
    with Image.open(path) as im:
        assert np.array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        write_png(path, img[..., :3])


N_CELLS, UMAP_KW = 60, dict(n_neighbors=5, n_epochs=20, seed=1)
COLORS = [(0.9, 0.1, 0.1), (0.1, 0.7, 0.2), (0.1, 0.2, 0.9)]


def _cells():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N_CELLS, 12)).astype(np.float32)
    md = pd.DataFrame({"tissue": [["lung", "gut", "skin"][i % 3] for i in range(N_CELLS)],
                       "donor": [f"d{i % 2}" for i in range(N_CELLS)]})
    return X, md


def _decode(path):
    from PIL import Image

    with Image.open(path) as im:
        return np.asarray(im.convert("RGBA")).copy()


def test_generate_umap_directory_forms(tmp_path):
    from mmvae_amd import backend, plots

    X, md = _cells()
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    np.savez(src / "z_embeddings.npz", embeddings=X)
    md.to_pickle(src / "z_metadata.pkl")
    kw = dict(decorate=False, colors=COLORS, width=64, height=48, umap_kw=UMAP_KW)
    with backend.cpu_plumbing():
        paths = plots.generate_umap(str(src), ("tissue", "donor"), ("z",), save_dir=str(out), **kw)
        assert paths == [str(out / "integrated.tissue.umap.z.png"), str(out / "integrated.donor.umap.z.png")]
        assert all(os.path.exists(p) for p in paths)
        stored = np.load(out / "z_umap_embeddings.npz")["embeddings"]
        assert stored.shape == (N_CELLS, 2) and pd.read_pickle(out / "z_umap_metadata.pkl").equals(md)
        first = _decode(paths[0])
        assert first.shape == (48, 64, 4) and (first[..., :3] != 255).any()
        # a second run over the output directory plots the stored embedding: no UMAP is fitted
        import mmvae_amd.umap as U

        def refuse(*a, **k):
            raise AssertionError("the stored embedding was not reused")

        orig, U.umap_embeddings = U.umap_embeddings, refuse
        try:
            again = plots.generate_umap(str(out), ("tissue",), ("z",), **kw)
        finally:
            U.umap_embeddings = orig
        assert again == [paths[0]] and np.array_equal(_decode(again[0]), first)
        want, _ = plots.rasterize(torch.from_numpy(stored).float(), plots.category_codes(md, "tissue")[0], 3, COLORS, 64, 48)
        assert np.array_equal(first, want.numpy())


def test_generate_umap_h5_form(tmp_path):
    from mmvae_amd import backend, plots
    from mmvae_amd import predictions as P

    X, md = _cells()
    h5 = str(tmp_path / "predictions.h5")
    P.save_to_hdf5(X, md, h5, "z")
    kw = dict(decorate=False, colors=COLORS, width=64, height=48, umap_kw=UMAP_KW)
    with backend.cpu_plumbing():
        paths = plots.generate_umap(h5, ("tissue",), ("z",), **kw)
        assert paths == [str(tmp_path / "integrated.tissue.umap.z.png")]
        emb = P.load_from_hdf5(h5, "z")[2]
        assert emb is not None and emb.shape == (N_CELLS, 2)
        first = _decode(paths[0])
        elsewhere = plots.generate_umap(h5, ("tissue",), ("z",), save_dir=str(tmp_path / "o"), **kw)
        assert elsewhere == [str(tmp_path / "o" / "integrated.tissue.umap.z.png")]
        assert np.array_equal(_decode(elsewhere[0]), first)  # from the embedding the first run stored
        assert np.array_equal(P.load_from_hdf5(h5, "z")[2], emb)
    with pytest.raises(FileNotFoundError):
        plots.generate_umap(str(tmp_path / "none.h5"), ("tissue",), ("z",))


def test_plot_category_decorated(tmp_path):
    pytest.importorskip("matplotlib")
    from mmvae_amd import backend, plots

    pts, codes = R.mixture(400, 3, 2, seed=3)
    md = pd.DataFrame({"tissue": np.array([b"lung", b"gut", b"skin"], dtype=object)[codes]})
    with backend.cpu_plumbing():
        path = plots.plot_category(pts, md, "tissue", str(tmp_path), 15, "z", "cmmvae")
        assert path == str(tmp_path / "integrated.tissue.umap.z.png")
        full = _decode(path)
        empty_md = pd.DataFrame({"tissue": [np.nan] * 400, "other": ["a"] * 400})
        # the same call with every code -1: no point is drawn (the legend differs too, the axes must)
        blank = plots.plot_category(pts, empty_md, "tissue", str(tmp_path / "blank"), 15, "z", "cmmvae")
        none = _decode(blank)
    assert full.ndim == 3 and full.shape[0] > 600 and full.shape[1] > 1085
    inside = full[100:500, 200:1000, :3]
    assert (inside != 255).any() and (none[100:500, 200:1000, :3] == 255).all()
    assert plots.palette(3)[0] == (0.0, 0.0, 0.0) and len(plots.palette(15)) == 15
    assert plots.marker_pixels(1) == 1 and plots.marker_pixels(4) == 3 and plots.marker_pixels(0.01) == 1


def test_tool_arguments(tmp_path, monkeypatch):
    import importlib.util

    spec = importlib.util.spec_from_file_location("umap_predictions_tool", os.path.join(ROOT, "tools", "umap_predictions.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.delenv("DIRECTORY", raising=False)
    a = tool.parse_args(["--directory", str(tmp_path), "--categories", "tissue", "--categories", "donor", "--keys", "z",
                         "--save_dir", "out", "--method", "cmmvae"])
    assert (a.directory, a.categories, a.keys, a.save_dir, a.method) == (str(tmp_path), ["tissue", "donor"], ["z"], "out",
                                                                         "cmmvae")
    b = tool.parse_args(["--directory", str(tmp_path), "--categories", "t", "--keys", "z", "--keys", "xhat"])
    assert b.save_dir is None and b.method == "" and b.keys == ["z", "xhat"]
    for bad in (["--categories", "t", "--keys", "z"], ["--directory", str(tmp_path), "--keys", "z"],
                ["--directory", str(tmp_path), "--categories", "t"],
                ["--directory", str(tmp_path / "missing"), "--categories", "t", "--keys", "z"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    # the whole tool on a stored embedding
    from mmvae_amd import backend

    X, md = _cells()
    np.savez(tmp_path / "z_umap_embeddings.npz", embeddings=X[:, :2])
    md.to_pickle(tmp_path / "z_umap_metadata.pkl")
    seen = {}
    import mmvae_amd.plots as plots

    monkeypatch.setattr(plots, "generate_umap", lambda *args, **kw: seen.update(args=args, kw=kw) or ["p.png"])
    with backend.cpu_plumbing():
        assert tool.main(["--directory", str(tmp_path), "--categories", "tissue", "--keys", "z"]) == 0
    assert seen["args"] == (str(tmp_path), ("tissue",), ("z",)) and seen["kw"] == {"method": "", "save_dir": None}
