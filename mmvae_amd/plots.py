"""Category scatter plots of an embedding, rasterised on the device: what `plot_category` / `generate_umap` of the
reference's runners/umap_predictions.py:53-253 produce through pandas and `plt.scatter`, as the two passes of
libmmvae_plot.so (include/mmvae_plot.h).

    category_codes   the reference's label selection (value_counts().nlargest(n_largest)) as int32 codes
    fit_view         the eight words of the affine data -> pixel map, with matplotlib's 5 % margins
    rasterize        per-pixel, per-class counts (HIP, integer atomics) and their composite (HIP) -> RGBA8
    write_png        an 8-bit RGBA PNG through zlib and struct
    plot_category    the reference's function: title, legend and file name; the raster is shown with imshow
    generate_umap    the reference's runner over a directory of npz/pkl pairs or a predictions.h5

Device tensors run the HIP kernels, always.  CPU tensors are refused outside `backend.cpu_plumbing()`; inside it
`rasterize` is its statement in numpy (`_rasterize_cpu`: pixel indices in float32 with the header's operation order,
the composite in fp64; tests/plot_restatement.py restates it independently).  Only `palette` and the decorated
`plot_category` import matplotlib.  Deviations from `plt.scatter` are listed in DESIGN.md: the expectation over drawing
orders instead of one shuffle, square markers instead of discs, no anti-aliasing.
"""
from __future__ import annotations

import math
import os
import struct
import sys
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _bind, backend
from ._plot_lib import PLOT_COUNT_DEFAULT, PLOT_MAX_CLASSES, PLOT_MAX_MARKER, PLOT_MAX_SIDE

FIGSIZE = (14, 8)          # the reference's plt.figure(figsize=(14, 8))
AXES_PIXELS = (1085, 616)  # the axes of that figure at matplotlib's default 100 dpi (plot_category asks matplotlib)


# ------------------------------------------------------------------------------------------------------------ labels
def category_codes(metadata, category: str, n_largest: int = 15) -> Tuple[np.ndarray, list]:
    """(codes int32 [N], labels): the labels are `metadata[category].value_counts().nlargest(n_largest).index` as the
    reference selects them, code i marks the rows of the i-th label and -1 every other row and every missing value.
    `bytes` labels (what load_from_hdf5 returns) are decoded in `labels`, which is for display."""
    column = metadata[category]
    chosen = column.value_counts().nlargest(n_largest).index
    if len(chosen) > PLOT_MAX_CLASSES:
        raise ValueError(f"category_codes: at most {PLOT_MAX_CLASSES} labels per picture (n_largest = {n_largest})")
    import pandas as pd

    codes = pd.Index(list(chosen), dtype=object).get_indexer(pd.Index(column.astype(object), dtype=object))
    labels = [v.decode("utf-8") if isinstance(v, bytes) else v for v in chosen]
    return np.ascontiguousarray(codes, dtype=np.int32), labels


# -------------------------------------------------------------------------------------------------------------- view
def view_matrix(elev: float = 30.0, azim: float = 0.0) -> List[List[float]]:
    """The 2 x 3 orthographic projection of a 3-component embedding seen from elevation `elev` and azimuth `azim`
    (degrees, mplot3d's angles: the reference's 3d_umap.py turns azim through 0 .. 359 at elev = 30): the first row is the
    screen's x direction, the second its y direction."""
    e, a = math.radians(elev), math.radians(azim)
    return [[-math.sin(a), math.cos(a), 0.0],
            [-math.sin(e) * math.cos(a), -math.sin(e) * math.sin(a), math.cos(e)]]


def _as_codes(codes, device) -> torch.Tensor:
    if not torch.is_tensor(codes):
        codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32))
    return codes.to(device=device, dtype=torch.int32).contiguous()


def _fit(points: torch.Tensor, codes, width: int, height: int, margin: float, matrix):
    """(view, (x0, x1, y0, y1)): the eight words and the data limits the picture's borders stand for."""
    backend.on_hip(points)
    if points.dim() != 2 or points.shape[1] not in (2, 3):
        raise ValueError(f"points must be [N, 2] or [N, 3], got {tuple(points.shape)}")
    dims = points.shape[1]
    if matrix is None:
        M = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    else:
        M = [[float(v) for v in row] + [0.0] * (3 - len(row)) for row in matrix]
        if len(M) != 2 or any(len(row) != 3 for row in M):
            raise ValueError("matrix: 2 rows of 2 or 3 numbers")
    codes = _as_codes(codes, points.device)
    P = points.double()
    proj = torch.stack([sum(M[r][j] * P[:, j] for j in range(dims)) for r in (0, 1)], 1)
    keep = (codes >= 0) & torch.isfinite(P).all(1) & torch.isfinite(proj).all(1)
    if bool(keep.any()):
        sel = proj[keep]
        lo, hi = sel.min(0).values.tolist(), sel.max(0).values.tolist()
    else:
        lo, hi = [0.0, 0.0], [1.0, 1.0]
    lim = []
    for a, b in zip(lo, hi):
        if b == a:  # a zero span is widened to one data unit around the value
            a, b = a - 0.5, b + 0.5
        pad = margin * (b - a)
        lim.append((a - pad, b + pad))
    (x0, x1), (y0, y1) = lim
    sx, sy = width / (x1 - x0), height / (y1 - y0)
    # u = sx (px - x0);  v = sy (y1 - py): the y axis points up, row 0 is the top of the picture
    view = [sx * M[0][0], sx * M[0][1], sx * M[0][2], -sx * x0, -sy * M[1][0], -sy * M[1][1], -sy * M[1][2], sy * y1]
    return view, (x0, x1, y0, y1)


def fit_view(points: torch.Tensor, codes, width: int, height: int, margin: float = 0.05, matrix=None) -> List[float]:
    """The eight view words (a00 a01 a02 b0 a10 a11 a12 b1 of include/mmvae_plot.h) that show the plotted points --
    code >= 0, finite coordinates -- with `margin` of their span free on every side (matplotlib's 0.05), the y axis
    pointing up.  Minimum and maximum are torch reductions on the points' device (plumbing).  `matrix` (2 x 3, e.g.
    `view_matrix`) projects a 3-component embedding first; without it the first two components are shown."""
    return _fit(points, codes, width, height, margin, matrix)[0]


# ------------------------------------------------------------------------------------------------------------ raster
def _rasterize_cpu(points: np.ndarray, codes: np.ndarray, n_classes: int, colors: np.ndarray, width: int, height: int,
                   view: Sequence[float], marker_px: int, alpha: float, background) -> Tuple[np.ndarray, np.ndarray]:
    """The statement of the two kernels in numpy: (rgba uint8 [H, W, 4], counts uint32 [C, H, W])."""
    f = np.float32
    a = [f(w) for w in view]
    P = np.asarray(points, dtype=f)
    dims = P.shape[1]
    with np.errstate(all="ignore"):
        u = a[0] * P[:, 0] + a[1] * P[:, 1]
        v = a[4] * P[:, 0] + a[5] * P[:, 1]
        if dims == 3:
            u = u + a[2] * P[:, 2]
            v = v + a[6] * P[:, 2]
        u, v = u + a[3], v + a[7]
        fu, fv = np.floor(u), np.floor(v)
    lo, hi = (marker_px - 1) // 2, marker_px // 2
    with np.errstate(invalid="ignore"):
        keep = ((codes >= 0) & (codes < n_classes) & np.isfinite(P).all(1) & np.isfinite(u) & np.isfinite(v)
                & (fu >= -hi) & (fu <= width - 1 + lo) & (fv >= -hi) & (fv <= height - 1 + lo))
    cx, cy, c = fu[keep].astype(np.int64), fv[keep].astype(np.int64), codes[keep].astype(np.int64)
    counts = np.zeros((n_classes, height, width), dtype=np.uint32)
    for dy in range(-lo, hi + 1):
        for dx in range(-lo, hi + 1):
            x, y = cx + dx, cy + dy
            inside = (x >= 0) & (x < width) & (y >= 0) & (y < height)
            np.add.at(counts, (c[inside], y[inside], x[inside]), 1)
    nc = counts.astype(np.float64)
    n = nc.sum(0)
    col = np.asarray(colors, dtype=f).astype(np.float64).reshape(n_classes, 3)
    bg = np.asarray([f(b) for b in background], dtype=np.float64)
    mean = np.einsum("chw,ck->hwk", nc, col) / np.maximum(n, 1.0)[..., None]
    t = ((1.0 - float(f(alpha))) ** n)[..., None]
    out = np.where(n[..., None] > 0, (1.0 - t) * mean + t * bg, bg)
    rgba = np.full((height, width, 4), 255, dtype=np.uint8)
    rgba[..., :3] = np.clip(np.rint(255.0 * out), 0, 255).astype(np.uint8)
    return rgba, counts


def rasterize(points: torch.Tensor, codes, n_classes: int, colors, width: int, height: int, view=None,
              marker_px: int = 1, alpha: float = 0.5, background=(1.0, 1.0, 1.0),
              count_mode: int = PLOT_COUNT_DEFAULT) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rgba uint8 [H, W, 4], counts [n_classes, H, W]) on the points' device: every point with a code in
    0 .. n_classes - 1 adds 1 to the `marker_px` x `marker_px` pixels around its place under `view` (default:
    `fit_view`) in the plane of its class, and every pixel becomes the expectation of alpha-blending its markers in
    `colors` [n_classes, 3] over `background` in a random order (include/mmvae_plot.h has both rules in full).  counts
    holds the kernel's uint32 words in an int32 tensor (a count stays below 2^31).  Enqueues on the current stream."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] not in (2, 3):
        raise ValueError("points: a tensor [N, 2] or [N, 3]")
    N, dims = points.shape
    n_classes, width, height, marker_px = int(n_classes), int(width), int(height), int(marker_px)
    if N < 1:
        raise ValueError("rasterize: no points")
    if not (1 <= n_classes <= PLOT_MAX_CLASSES and 1 <= width <= PLOT_MAX_SIDE and 1 <= height <= PLOT_MAX_SIDE
            and 1 <= marker_px <= PLOT_MAX_MARKER):
        raise ValueError(f"rasterize: need 1 <= n_classes <= {PLOT_MAX_CLASSES}, sides of 1 .. {PLOT_MAX_SIDE} and a marker "
                         f"of 1 .. {PLOT_MAX_MARKER} pixels (got {n_classes}, {width} x {height}, {marker_px})")
    if not 0.0 < float(alpha) <= 1.0 or not all(0.0 <= float(b) <= 1.0 for b in background) or len(background) != 3:
        raise ValueError("rasterize: alpha in (0, 1] and three background channels in [0, 1]")
    on_hip = backend.on_hip(points)
    codes = _as_codes(codes, points.device)
    if codes.shape != (N,):
        raise ValueError(f"rasterize: {N} points, codes of shape {tuple(codes.shape)}")
    if view is None:
        view = fit_view(points, codes, width, height)
    colors = torch.as_tensor(colors, dtype=torch.float32).reshape(-1, 3)
    if colors.shape[0] != n_classes:
        raise ValueError(f"rasterize: {n_classes} classes, {colors.shape[0]} colours")
    if not on_hip:
        rgba, counts = _rasterize_cpu(points.detach().float().numpy(), codes.numpy(), n_classes, colors.cpu().numpy(),
                                      width, height, view, marker_px, float(alpha), background)
        return torch.from_numpy(rgba), torch.from_numpy(counts.view(np.int32))
    from . import _plot_lib

    if points.dtype != torch.float32:
        raise TypeError(f"rasterize: expected float32 points, got {points.dtype}")
    if points.stride(1) != 1:
        points = points.contiguous()
    ld = points.stride(0) if N > 1 else dims
    lib = _plot_lib.load_plot()
    dev = points.device
    colors = colors.to(dev).contiguous()
    counts = torch.empty((n_classes, height, width), dtype=torch.int32, device=dev)
    rgba = torch.empty((height, width, 4), dtype=torch.uint8, device=dev)
    stream = _bind.stream(dev)
    _plot_lib.check(lib.mmvae_plot_count_f32(N, dims, points.data_ptr(), ld, codes.data_ptr(), n_classes, width, height,
                                             marker_px, _plot_lib.view_words(view), int(count_mode), counts.data_ptr(),
                                             stream), "mmvae_plot_count_f32")
    _plot_lib.check(lib.mmvae_plot_composite_u8(counts.data_ptr(), n_classes, width, height, colors.data_ptr(),
                                                float(alpha), float(background[0]), float(background[1]),
                                                float(background[2]), rgba.data_ptr(), stream), "mmvae_plot_composite_u8")
    return rgba, counts


# --------------------------------------------------------------------------------------------------------------- PNG
def write_png(path: str, rgba) -> None:
    """`rgba` [H, W, 4] uint8 (tensor or array) as an 8-bit RGBA PNG: zlib and struct only."""
    if torch.is_tensor(rgba):
        rgba = rgba.detach().cpu().numpy()
    img = np.ascontiguousarray(rgba)
    if img.ndim != 3 or img.shape[2] != 4 or img.dtype != np.uint8 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"write_png: expected uint8 [H, W, 4], got {img.dtype} {img.shape}")
    H, W = img.shape[:2]
    rows = np.zeros((H, 1 + 4 * W), dtype=np.uint8)  # every row behind its filter byte 0 (none)
    rows[:, 1:] = img.reshape(H, 4 * W)

    def chunk(kind: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


# ------------------------------------------------------------------------------------------------------------- plots
def palette(n: int) -> List[Tuple[float, float, float]]:
    """The RGB of the n colours of `plt.get_cmap("nipy_spectral", n)`, the reference's colour list."""
    import matplotlib

    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt

    cmap = plt.get_cmap("nipy_spectral", n)
    return [tuple(float(ch) for ch in cmap(i)[:3]) for i in range(n)]


def _as_points(embedding) -> torch.Tensor:
    """A tensor stays where it is; an array goes to the GPU -- or stays on the host inside backend.cpu_plumbing()."""
    if torch.is_tensor(embedding):
        return embedding.detach().float()
    t = torch.from_numpy(np.ascontiguousarray(embedding, dtype=np.float32))
    return t if backend.cpu_plumbing_enabled() else t.cuda()


def marker_pixels(marker_size: float, dpi: float = 100.0) -> int:
    """The side in pixels of a scatter marker of area `marker_size` points^2: max(1, round(sqrt(marker_size) dpi / 72))."""
    return max(1, int(round(math.sqrt(marker_size) * dpi / 72.0)))


def plot_category(embedding, metadata, category: str, save_path: str, n_largest: int, name: str, method: str,
                  alpha: float = 0.5, marker_size: float = 1, *, decorate: bool = True, colors=None, matrix=None,
                  width: Optional[int] = None, height: Optional[int] = None) -> str:
    """The reference's plot_category: the embedding's points of the `n_largest` most common labels of
    `metadata[category]`, coloured by label, as `save_path`/integrated.{category}.umap.{name}.png; returns that path.
    The points are rasterised on the embedding's device at the pixel size of the axes (asked of matplotlib for the
    reference's 14 x 8 in figure; `width`, `height` override) and shown with imshow under the axes' data extent, below
    the reference's title and legend.  `decorate=False` writes the bare raster with `write_png` and needs no matplotlib
    when `colors` [labels, 3] is given (default: `palette`).  `matrix`: see `fit_view`, for 3 components."""
    points = _as_points(embedding)
    codes, labels = category_codes(metadata, category, n_largest)
    if len(codes) != points.shape[0]:
        raise ValueError(f"plot_category: {points.shape[0]} points, {len(codes)} metadata rows")
    n_classes = max(1, len(labels))
    if colors is None:
        colors = palette(n_classes)
    colors = [tuple(float(ch) for ch in c[:3]) for c in colors]
    if len(colors) < n_classes:
        raise ValueError(f"plot_category: {n_classes} labels, {len(colors)} colours")
    colors = colors[:n_classes]
    os.makedirs(save_path, exist_ok=True)
    image_path = os.path.join(save_path, f"integrated.{category}.umap.{name}.png")
    if not decorate:
        W, H = int(width or AXES_PIXELS[0]), int(height or AXES_PIXELS[1])
        view, _ = _fit(points, codes, W, H, 0.05, matrix)
        rgba, _ = rasterize(points, codes, n_classes, colors, W, H, view, marker_pixels(marker_size), alpha)
        write_png(image_path, rgba)
        return image_path

    import matplotlib

    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt

    fig = plt.figure(figsize=FIGSIZE)
    try:
        ax = fig.gca()
        box = ax.get_window_extent()
        W, H = int(width or round(box.width)), int(height or round(box.height))
        view, extent = _fit(points, codes, W, H, 0.05, matrix)
        rgba, _ = rasterize(points, codes, n_classes, colors, W, H, view, marker_pixels(marker_size, fig.dpi), alpha)
        ax.imshow(rgba.cpu().numpy(), extent=extent, interpolation="nearest", aspect="auto", origin="upper")
        ax.set_title(f"UMAP projection{f' for {method} ' if method else ' '}colored by {category}")
        handles = [plt.Line2D([0], [0], marker="o", color="w", label=label, markerfacecolor=colors[i], markersize=10)
                   for i, label in enumerate(labels)]
        ax.legend(handles=handles, title=category, bbox_to_anchor=(1.05, 1), loc="upper left")
        fig.savefig(image_path, bbox_inches="tight")
    finally:
        plt.close(fig)
    return image_path


def _load_pair(npz_path: str, meta_path: str):
    import pandas as pd

    return np.load(npz_path)["embeddings"], pd.read_pickle(meta_path)


def generate_umap(directory: str, categories: Sequence[str], keys: Sequence[str], method: str = "",
                  save_dir: Optional[str] = None, n_largest: int = 15, umap_kw: Optional[dict] = None,
                  **plot_kw) -> List[str]:
    """The reference's generate_umap with both of its input forms; returns the image paths, keys outermost.

    A directory: `{key}_umap_embeddings.npz` with `{key}_umap_metadata.pkl` is plotted as stored; otherwise
    `{key}_embeddings.npz` with `{key}_metadata.pkl` is embedded by `umap.umap_embeddings` on the device and the pair is
    saved under those names in `save_dir` (default: the directory), as plot_umap does.  A path ending in ".h5": group
    `key` through `predictions.load_from_hdf5`; a missing embedding is computed and stored with
    `predictions.write_umap_embeddings`; `save_dir` defaults to the file's directory.  `umap_kw` goes to umap_embeddings (default: the
    reference's settings), `plot_kw` to plot_category."""
    from .umap import umap_embeddings

    umap_kw = dict(umap_kw or {})

    image_paths: List[str] = []
    if directory.endswith(".h5"):
        from . import predictions as P

        if not os.path.exists(directory):
            raise FileNotFoundError(directory)
        save_dir = save_dir or os.path.dirname(directory)
        for key in keys:
            data, metadata, embedding = P.load_from_hdf5(directory, key)
            if embedding is None:
                embedding = umap_embeddings(_as_points(data), **umap_kw)
                P.write_umap_embeddings(directory, key, embedding)
            image_paths += [plot_category(embedding, metadata, c, save_dir, n_largest, key, method, **plot_kw)
                            for c in categories]
        return image_paths
    save_dir = save_dir or directory
    for key in keys:
        stored = os.path.join(directory, f"{key}_umap_embeddings.npz")
        if os.path.exists(stored):
            embedding, metadata = _load_pair(stored, os.path.join(directory, f"{key}_umap_metadata.pkl"))
        else:
            X, metadata = _load_pair(os.path.join(directory, f"{key}_embeddings.npz"),
                                     os.path.join(directory, f"{key}_metadata.pkl"))
            sys.stderr.write("Fitting umap embeddings...\n")
            embedding = umap_embeddings(_as_points(X), **umap_kw)
            os.makedirs(save_dir, exist_ok=True)
            np.savez(os.path.join(save_dir, f"{key}_umap_embeddings.npz"), embeddings=embedding.cpu().numpy())
            metadata.to_pickle(os.path.join(save_dir, f"{key}_umap_metadata.pkl"))
        image_paths += [plot_category(embedding, metadata, c, save_dir, n_largest, key, method, **plot_kw)
                        for c in categories]
    return image_paths
