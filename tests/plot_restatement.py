"""An independent numpy statement of libmmvae_plot.so (include/mmvae_plot.h), no torch: pixel indices in float32 with
the header's operation order, counts through np.add.at, the composite in fp64.  The tests compute it once per case and
never modify it."""
import itertools

import numpy as np

F = np.float32


def pixel_centres(points, view):
    """(u, v) float32 and the centre pixels as float32 floors: every product and every sum rounded to float32 on its
    own, in the order  ((a00 x + a01 y) [+ a02 z]) + b0."""
    p = np.asarray(points, dtype=F)
    w = np.asarray(view, dtype=F)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        u = np.add(np.multiply(w[0], x, dtype=F), np.multiply(w[1], y, dtype=F), dtype=F)
        v = np.add(np.multiply(w[4], x, dtype=F), np.multiply(w[5], y, dtype=F), dtype=F)
        if p.shape[1] == 3:
            u = np.add(u, np.multiply(w[2], p[:, 2], dtype=F), dtype=F)
            v = np.add(v, np.multiply(w[6], p[:, 2], dtype=F), dtype=F)
        u = np.add(u, w[3], dtype=F)
        v = np.add(v, w[7], dtype=F)
        return u, v, np.floor(u), np.floor(v)


def count(points, codes, n_classes, width, height, marker, view):
    """counts uint32 [n_classes, height, width]."""
    p = np.asarray(points, dtype=F)
    codes = np.asarray(codes, dtype=np.int64)
    u, v, fu, fv = pixel_centres(p, view)
    left, right = (marker - 1) // 2, marker // 2  # the block: cx - left .. cx + right
    flat = np.zeros(n_classes * height * width, dtype=np.uint32)
    for i in range(len(p)):
        if not 0 <= codes[i] < n_classes:
            continue
        if not (np.isfinite(p[i]).all() and np.isfinite(u[i]) and np.isfinite(v[i])):
            continue
        if not (-right <= fu[i] <= width - 1 + left and -right <= fv[i] <= height - 1 + left):
            continue
        cx, cy = int(fu[i]), int(fv[i])
        xs = [x for x in range(cx - left, cx + right + 1) if 0 <= x < width]
        ys = [y for y in range(cy - left, cy + right + 1) if 0 <= y < height]
        idx = [(codes[i] * height + y) * width + x for y in ys for x in xs]
        np.add.at(flat, idx, 1)
    return flat.reshape(n_classes, height, width)


def composite_exact(counts, colors, alpha, background):
    """[H, W, 3] fp64: 255 x the expected colour, before rounding.  alpha and the colours as the float32 the ABI takes."""
    nc = np.asarray(counts).astype(np.float64)
    n = nc.sum(0)
    col = np.asarray(colors, dtype=F).astype(np.float64).reshape(len(nc), 3)
    bg = np.asarray(background, dtype=F).astype(np.float64)
    keep = (1.0 - float(F(alpha))) ** n
    safe = np.where(n > 0, n, 1.0)
    mean = np.tensordot(nc, col, axes=([0], [0])) / safe[..., None]
    out = (1.0 - keep)[..., None] * mean + keep[..., None] * bg
    out[n == 0] = bg
    return 255.0 * out


def composite(counts, colors, alpha, background):
    """rgba uint8 [H, W, 4]."""
    exact = composite_exact(counts, colors, alpha, background)
    rgba = np.full(exact.shape[:2] + (4,), 255, dtype=np.uint8)
    rgba[..., :3] = np.clip(np.rint(exact), 0, 255).astype(np.uint8)
    return rgba


def blend_in_order(colors_in_order, alpha, background):
    """One draw of the reference's picture for one pixel: the markers alpha-blended over the background in this order."""
    out = np.asarray(background, dtype=np.float64)
    for c in colors_in_order:
        out = alpha * np.asarray(c, dtype=np.float64) + (1.0 - alpha) * out
    return out


def mean_over_orders(point_colors, alpha, background):
    """The mean of blend_in_order over every order of the points."""
    orders = list(itertools.permutations(range(len(point_colors))))
    return sum(blend_in_order([point_colors[i] for i in o], alpha, background) for o in orders) / len(orders)


def mixture(n, n_classes=15, dims=2, seed=0, spread=0.35):
    """A seeded Gaussian-mixture embedding: (points float32 [n, dims], codes int32 [n]), class c around its own centre."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-8.0, 8.0, size=(n_classes, dims))
    codes = rng.integers(0, n_classes, size=n).astype(np.int32)
    pts = centres[codes] + spread * rng.standard_normal((n, dims))
    return pts.astype(F), codes
