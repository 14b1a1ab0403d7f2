"""libmmvae_plot.so on the GPU against the numpy restatement (tests/plot_restatement.py).

Counts are integers and the pixel index is stated operation by operation in float32, so every count comparison is
exact.  Composite bound: the kernel evaluates the closed form in fp32; its value differs from the fp64 restatement by a
few 2^-24 x 255, so a channel may fall on the other side of a rounding boundary -- by 1, never more: the bound is 1, and
the share of channels that differ at all is printed.  Where a value is further than 1e-3 from every boundary (fp32 error
of 255 x a mean of at most 16 terms <= 255 x 20 x 2^-24 = 3e-4) the channel must be equal."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import plot_restatement as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (37, 23), (256, 64)]
NS = [1, 63, 64, 65, 1031]
CLASS_MARKER = [(c, m) for c in (1, 15, 16) for m in (1, 2, 3, 8)]
# how the points lie in memory: (dims, leading dimension, element offset of the first point)
#   packed and 16-byte aligned: the four-points-per-lane loads;  a wider row or a base off 16 bytes: element by element
LAYOUTS = [(2, 2, 0), (2, 5, 0), (3, 3, 0), (3, 4, 0), (2, 2, 1), (3, 3, 2)]


def on_device(pts, ld, offset=0):
    """pts on the GPU as a view with leading dimension ld, its first element `offset` elements into an allocation."""
    n, d = pts.shape
    buf = torch.full((offset + n * ld + 8,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[offset:offset + n * ld].view(n, ld)[:, :d]
    view.copy_(torch.from_numpy(pts))
    return view


def device_counts(pts, codes, C, W, H, m, view, layout=(2, 2, 0), mode=0):
    from mmvae_amd import plots

    dims, ld, off = layout
    assert pts.shape[1] == dims
    colors = np.zeros((C, 3), np.float32)
    _, counts = plots.rasterize(on_device(pts, ld, off), torch.from_numpy(codes).cuda(), C, colors, W, H, view=view,
                                marker_px=m, count_mode=mode)
    return counts.cpu().numpy().view(np.uint32)


def spread_view(pts, codes, W, H, dims):
    """A view that shows the middle 3/4 of the spread, turned for 3 components: markers are clipped at, and fall off,
    every border."""
    from mmvae_amd import backend, plots

    with backend.cpu_plumbing():
        v = plots.fit_view(torch.from_numpy(pts), codes, W, H, matrix=plots.view_matrix(30, 40) if dims == 3 else None)
    cx, cy = W / 2.0, H / 2.0
    s = 4.0 / 3.0  # scale about the picture's centre
    return [s * v[0], s * v[1], s * v[2], s * (v[3] - cx) + cx, s * v[4], s * v[5], s * v[6], s * (v[7] - cy) + cy]


@pytest.mark.parametrize("W, H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("N", NS)
def test_counts_equal_the_restatement(N, W, H):
    """Every (n_classes, marker) pair at this N and picture size; the memory layouts and the two ways of adding take
    turns over the pairs (each layout meets each pair at some N), and both ways of adding run on every case."""
    case = NS.index(N) * len(SIZES) + SIZES.index((W, H))
    clipped = 0
    for i, (C, m) in enumerate(CLASS_MARKER):
        layout = LAYOUTS[(i + case) % len(LAYOUTS)]
        dims = layout[0]
        pts, codes = R.mixture(N, C, dims, seed=1000 * case + i)
        view = spread_view(pts, codes, W, H, dims)
        want = R.count(pts, codes, C, W, H, m, view)
        for mode in (1, 2):
            got = device_counts(pts, codes, C, W, H, m, view, layout, mode)
            assert np.array_equal(got, want), (N, W, H, C, m, layout, mode)
        assert want.sum() > 0 or N < 63
        clipped += int(want.sum() < N * m * m)
    if N >= 63:
        assert clipped > 0  # some markers lay across or beyond a border


@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_borders_boundaries_and_block_placement(m):
    """The identity view on a 37 x 23 picture: points exactly on pixel boundaries, in the four corners, on the far edges
    (u = W, v = H: one pixel outside) and just outside, so that blocks are clipped at all four borders.  The block of an
    even marker reaches further right and down: pinned here on one point in the middle."""
    W, H = 37, 23
    identity = [1, 0, 0, 0, 0, 1, 0, 0]
    xs = [-4.0, -3.5, -1.0, -0.0, 0.0, 0.5, 1.0, 17.999999, 18.0, 36.0, 36.999996, 37.0, 38.5, 40.0, 41.0]
    ys = [-4.0, -1.0, -1e-7, 0.0, 1.0, 11.0, 22.0, 22.999998, 23.0, 25.0, 26.0, 27.0]
    pts = np.array([(x, y) for x in xs for y in ys], np.float32)
    codes = (np.arange(len(pts)) % 3).astype(np.int32)
    want = R.count(pts, codes, 3, W, H, m, identity)
    for mode in (1, 2):
        assert np.array_equal(device_counts(pts, codes, 3, W, H, m, identity, mode=mode), want)
    assert want[:, 0, :].any() and want[:, H - 1, :].any() and want[:, :, 0].any() and want[:, :, W - 1].any()
    one = device_counts(np.array([[10.25, 7.75]], np.float32), np.zeros(1, np.int32), 1, W, H, m, identity)[0]
    rows, cols = np.nonzero(one)
    left, right = (m - 1) // 2, m // 2
    assert one.sum() == m * m and one.max() == 1
    assert (cols.min(), cols.max(), rows.min(), rows.max()) == (10 - left, 10 + right, 7 - left, 7 + right)
    # a point ON the far edge lies in the pixel outside: gone for m = 1 and 2, for m = 3 and 8 its block reaches back in
    edge = device_counts(np.array([[37.0, 5.0]], np.float32), np.zeros(1, np.int32), 1, W, H, m, identity)[0]
    assert edge.sum() == left * m and (left == 0 or edge[:, W - left:].sum() == edge.sum())


def test_dropped_points_leave_no_trace():
    W, H, C = 37, 23, 15
    big = np.float32(1e38)
    for dims, layout in ((2, (2, 2, 0)), (3, (3, 3, 0)), (3, (3, 4, 0))):
        clean, ccodes = R.mixture(200, C, dims, seed=5)
        view = spread_view(clean, ccodes, W, H, dims)
        bad_rows, bad_codes = [], []
        for code in (-1, C, np.iinfo(np.int32).min, np.iinfo(np.int32).max, 16, -2 ** 30):
            bad_rows.append(clean[len(bad_rows)])  # a visible place with a code that is none
            bad_codes.append(code)
        for value in (np.nan, np.inf, -np.inf, big, -big):
            for axis in range(dims):
                row = clean[len(bad_rows)].copy()
                row[axis] = value
                bad_rows.append(row)
                bad_codes.append(3)
        bad_rows.append(np.full(dims, big, np.float32))
        bad_codes.append(0)
        order = np.random.default_rng(0).permutation(200 + len(bad_rows))
        pts = np.concatenate([clean, np.array(bad_rows, np.float32)])[order]
        codes = np.concatenate([ccodes, np.array(bad_codes, np.int64).astype(np.int32)])[order]
        want = R.count(clean, ccodes, C, W, H, 3, view)
        assert np.array_equal(R.count(pts, codes, C, W, H, 3, view), want)
        for mode in (1, 2):
            assert np.array_equal(device_counts(pts, codes, C, W, H, 3, view, layout, mode), want), (dims, layout, mode)


def test_contention_100000_points_on_one_pixel():
    W, H = 37, 23
    pts = np.tile(np.array([[12.5, 3.5]], np.float32), (100000, 1))
    codes = np.full(100000, 2, np.int32)
    for mode in (0, 1, 2):
        got = device_counts(pts, codes, 4, W, H, 1, [1, 0, 0, 0, 0, 1, 0, 0], mode=mode)
        assert got[2, 3, 12] == 100000 and got.sum() == 100000, mode


def test_calls_are_bit_identical_dirty_buffer_and_stream():
    from mmvae_amd import _plot_lib, plots

    W, H, C, N = 256, 64, 15, 1031
    pts, codes = R.mixture(N, C, 2, seed=9)
    view = spread_view(pts, codes, W, H, 2)
    want = R.count(pts, codes, C, W, H, 2, view)
    lib = _plot_lib.load_plot()
    p, c = torch.from_numpy(pts).cuda(), torch.from_numpy(codes).cuda()
    buf = torch.full((C, H, W), 0x7f7f7f7f, dtype=torch.int32, device="cuda")  # a dirty buffer: the entry clears it
    words = _plot_lib.view_words(view)
    outs = []
    for _ in range(2):
        rc = lib.mmvae_plot_count_f32(N, 2, p.data_ptr(), 2, c.data_ptr(), C, W, H, 2, words, 0, buf.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == _plot_lib.OK
        outs.append(buf.cpu().numpy().view(np.uint32).copy())
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    colors = np.random.default_rng(0).uniform(0, 1, (C, 3)).astype(np.float32)
    with torch.cuda.stream(side):
        rgba, counts = plots.rasterize(p, c, C, colors, W, H, view=view, marker_px=2)
    side.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want)
    assert np.abs(rgba.cpu().numpy().astype(int) - R.composite(want, colors, 0.5, (1, 1, 1)).astype(int)).max() <= 1


def _composite_on_device(counts, colors, alpha, bg):
    from mmvae_amd import _plot_lib

    C, H, W = counts.shape
    lib = _plot_lib.load_plot()
    cd = torch.from_numpy(counts.view(np.int32)).cuda()
    col = torch.from_numpy(np.asarray(colors, np.float32)).cuda()
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    rc = lib.mmvae_plot_composite_u8(cd.data_ptr(), C, W, H, col.data_ptr(), alpha, bg[0], bg[1], bg[2], out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == _plot_lib.OK
    return out.cpu().numpy()


@pytest.mark.parametrize("C, W, H", [(1, 1, 1), (15, 37, 23), (16, 256, 64), (15, 300, 7)])
def test_composite_against_fp64(C, W, H):
    rng = np.random.default_rng(C * W)
    # counts from 0 to large: empty pixels, a few points (the blend matters), many (saturated) and huge single counts
    counts = rng.integers(0, 4, (C, H, W)).astype(np.uint32) * (rng.random((C, H, W)) < 0.3)
    counts[:, rng.random((H, W)) < 0.2] = 0
    heavy = rng.random((H, W)) < 0.1
    counts[0, heavy] = rng.integers(1, 3_000_000, int(heavy.sum()))
    counts = counts.astype(np.uint32)
    colors = rng.uniform(0, 1, (C, 3)).astype(np.float32)
    for alpha, bg in ((0.5, (1.0, 1.0, 1.0)), (0.3, (0.1, 0.5, 0.9)), (1.0, (0.0, 0.0, 0.0)), (0.02, (1.0, 0.5, 0.25))):
        got = _composite_on_device(counts, colors, alpha, bg)
        exact = R.composite_exact(counts, colors, alpha, bg)
        want = R.composite(counts, colors, alpha, bg)
        diff = np.abs(got[..., :3].astype(int) - want[..., :3].astype(int))
        share = float((diff > 0).mean())
        print(f"composite {C} x {H} x {W} alpha {alpha}: {100 * share:.3f} % of channels differ from the fp64 rounding, "
              f"largest difference {diff.max()}")
        assert (got[..., 3] == 255).all() and diff.max() <= 1
        firm = np.abs(exact - np.floor(exact) - 0.5) > 1e-3  # further than the fp32 error from a rounding boundary
        assert np.array_equal(got[..., :3][firm], want[..., :3][firm])
        empty = counts.sum(0) == 0
        assert (got[empty][:, :3] == np.rint(255.0 * np.asarray(bg, np.float32).astype(np.float64)).astype(np.uint8)).all()
        if alpha == 1.0:  # exactly the rounded mean colour: a single class gives its colour whatever its count
            single = (counts[0] > 0) & (counts[1:].sum(0) == 0)
            if single.any():
                c0 = np.rint(255.0 * colors[0].astype(np.float64)).astype(np.uint8)
                f0 = np.abs(255.0 * colors[0].astype(np.float64) % 1.0 - 0.5) > 1e-3
                assert (got[single][:, :3][:, f0] == c0[f0]).all()


def test_device_tensors_never_take_the_cpu_path(monkeypatch):
    from mmvae_amd import backend, plots

    def refuse(*a, **k):
        raise AssertionError("a device tensor reached the numpy statement")

    monkeypatch.setattr(plots, "_rasterize_cpu", refuse)
    pts, codes = R.mixture(500, 15, 2, seed=2)
    colors = np.random.default_rng(0).uniform(0, 1, (15, 3)).astype(np.float32)
    for ctx in (backend.cpu_plumbing(False), backend.cpu_plumbing(True)):  # not even when plumbing is switched on
        with ctx:
            rgba, counts = plots.rasterize(torch.from_numpy(pts).cuda(), codes, 15, colors, 64, 48)
            assert rgba.is_cuda and counts.is_cuda and int(counts.sum()) == 500
    with pytest.raises(AssertionError, match="numpy statement"), backend.cpu_plumbing():
        plots.rasterize(torch.from_numpy(pts), codes, 15, colors, 64, 48)


def test_trainer_umap_plots_writes_the_raster(tmp_path, monkeypatch):
    from PIL import Image

    from mmvae_amd import plots
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
    batches = [((x * float(s)).cuda(), pd.DataFrame({"tissue": [["lung", "gut", "skin"][(i + j) % 3] for i in range(B)],
                                                     "donor": [f"d{i % 2}" for i in range(B)]}), eid)
               for j, s in enumerate(rng.uniform(0.5, 1.5, 4))]
    colors = [(0.9, 0.1, 0.1), (0.1, 0.7, 0.2), (0.1, 0.2, 0.9)]
    kw = dict(n_neighbors=5, n_epochs=30, seed=3)
    out = tmp_path / "plots"
    kept, umap = {}, Trainer.umap

    def keep(self, *a, **k):
        kept["out"] = umap(self, *a, **k)
        return kept["out"]

    monkeypatch.setattr(Trainer, "umap", keep)
    paths = Trainer().umap_plots(model, batches, ("tissue", "donor"), str(out), key="z",
                                 plot_kw=dict(decorate=False, colors=colors, marker_size=4), **kw)
    assert paths == [str(out / "integrated.tissue.umap.z.png"), str(out / "integrated.donor.umap.z.png")]
    emb, metadata = kept["out"]  # the embedding the pictures were made from
    assert emb.is_cuda and emb.shape == (4 * B, 2)
    for path, category, n in zip(paths, ("tissue", "donor"), (3, 2)):
        codes, labels = plots.category_codes(metadata, category)
        assert len(labels) == n
        want, counts = plots.rasterize(emb, codes, n, colors[:n], 1085, 616, marker_px=plots.marker_pixels(4))
        with Image.open(path) as im:
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), want.cpu().numpy())
        assert int(counts.sum()) == 4 * B * 9  # every cell's 3 x 3 marker lies inside the margins
