"""Inputs and restatements shared by tests/test_grad_hist_host.py and tests/test_grad_hist_gpu.py."""
import numpy as np

SENTINEL = np.float32(3.0e7)  # fills every gap of the geometry case: a value no segment contains


def edge_neighbour_values(edges: np.ndarray) -> np.ndarray:
    """For every edge its round-to-nearest fp32 value and that value's fp32 neighbours on both sides; +-0, +- the
    smallest denormal, +-FLT_MAX, NaN and +-inf; 1e30 (above the last edge) and -1e30."""
    e32 = edges.astype(np.float32)
    up = np.nextafter(e32, np.float32(np.inf))
    down = np.nextafter(e32, np.float32(-np.inf))
    tiny = np.float32(1e-45)
    fmax = np.finfo(np.float32).max
    extra = np.array([0.0, -0.0, tiny, -tiny, fmax, -fmax, np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=np.float32)
    return np.concatenate([e32, up, down, extra]).astype(np.float32)


def reference(values: np.ndarray, offsets, lengths, edges: np.ndarray, scale=None):
    """(counts [S, n_edges - 1] int64, stats [S, 8] fp64) by np.histogram per segment, in fp64, of the finite values;
    `scale`: multiplied in fp32 first."""
    counts = np.zeros((len(offsets), len(edges) - 1), dtype=np.int64)
    stats = np.zeros((len(offsets), 8), dtype=np.float64)
    for s, (o, n) in enumerate(zip(offsets, lengths)):
        v = values[o:o + n]
        if scale is not None:
            v = (v * np.float32(scale)).astype(np.float32)
        f = v[np.isfinite(v)].astype(np.float64)
        counts[s] = np.histogram(f, bins=edges)[0]
        stats[s] = (f.min() if f.size else np.inf, f.max() if f.size else -np.inf, f.size, f.sum(), (f * f).sum(),
                    n - f.size, (f < edges[0]).sum(), (f > edges[-1]).sum())
    return counts, stats


def geometry_case(C: int, seed: int = 7):
    """(values, offsets, lengths): segments of 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1 and 3C + 7
    elements whose start offsets cover all four residues mod 4, every gap and both ends filled with SENTINEL; the
    values are normal x 10^uniform(-8, 2) with both signs and 30 % exact zeros."""
    rng = np.random.default_rng(seed)
    lengths = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 7]
    offsets, pos = [], 5
    for i, n in enumerate(lengths):
        pos += (i % 4 - pos) % 4 + 4  # a gap of 4 .. 7 sentinels, start residue i mod 4
        offsets.append(pos)
        pos += n
    total = pos + 9
    values = np.full(total, SENTINEL, dtype=np.float32)
    for o, n in zip(offsets, lengths):
        v = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 2, n)
        v[rng.random(n) < 0.3] = 0.0
        values[o:o + n] = v.astype(np.float32)
    assert {o % 4 for o in offsets} == {0, 1, 2, 3}
    return values, offsets, lengths


def tensorboard_raw_restatement(counts, edges, stats_row):
    """What SegmentHistograms.tensorboard_raw must give, written from the description of make_histogram's trimming: walk
    to the first and the last non-empty bucket, keep them and everything between, put the bucket to the left of the
    first in front (a zero when there is none), and give the right edge of every kept bucket -- for the prepended zero
    that is the left edge of the first bucket."""
    counts = [int(c) for c in counts]
    filled = [i for i, c in enumerate(counts) if c > 0]
    if not filled:
        return None
    first, last = filled[0], filled[-1]
    kept, limits = [], []
    if first == 0:
        kept.append(0)
        limits.append(float(edges[0]))
    else:
        kept.append(counts[first - 1])
        limits.append(float(edges[first]))
    for i in range(first, last + 1):
        kept.append(counts[i])
        limits.append(float(edges[i + 1]))
    return {"min": float(stats_row[0]), "max": float(stats_row[1]), "num": int(stats_row[2]), "sum": float(stats_row[3]),
            "sum_squares": float(stats_row[4]), "bucket_limits": limits, "bucket_counts": kept}
