"""Segmented histograms of a flat fp32 tensor: every parameter's gradient histogram from one pass over an optimiser's
gradient arena (libmmvae_hist.so, include/mmvae_hist.h).

The reference's `save_gradients()` (models/base_model.py:178-231) gives each gradient tensor to
`SummaryWriter.add_histogram`, which copies it to the host and runs `np.histogram` over TensorBoard's 1 549 default
edges.  Here the arena is read once on the device; what reaches the host is the bucket counts and eight numbers per
parameter, and `SegmentHistograms.tensorboard_raw` shapes them as the arguments of `SummaryWriter.add_histogram_raw`.

Device tensors go through the library -- missing, it raises: no torch fallback.  CPU tensors go through numpy
(`_segment_histograms_cpu`): the host tests and CPU models run on it, and it states the semantics.

Deviation from `torch.utils.tensorboard.summary.make_histogram`: there `min`, `max`, `sum` and `sum_squares` run over
all values and turn NaN with one non-finite gradient, `num` counts all values, and an input without a value inside the
edges raises.  Here the moments describe the FINITE values, `num` is their count, `n_nonfinite` says how many were
not finite, and `tensorboard_raw` returns None when no finite value fell into a bucket.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _hist_lib
from ._bind import stream
from ._hist_lib import HIST_ITEM_DTYPE, HIST_ITEM_ELEMS, HIST_MAX_EDGES, HIST_STAT_NAMES, HIST_STATS

_TB_EDGES: Optional[np.ndarray] = None


def tensorboard_edges() -> np.ndarray:
    """The 1 549 default bucket edges of TensorBoard's bins="tensorflow" (fp64): 774 positive edges 1e-12 * 1.1^k below
    1e20, their negatives in reverse in front of them and 0.0 in between."""
    global _TB_EDGES
    if _TB_EDGES is None:
        pos = []
        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        _TB_EDGES = np.asarray([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)
        _TB_EDGES.setflags(write=False)
    return _TB_EDGES


def check_edges(edges) -> np.ndarray:
    """`edges` as a 1-D fp64 array of 2 .. HIST_MAX_EDGES strictly ascending finite values, or ValueError."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
    if e.ndim != 1 or not 2 <= e.size <= HIST_MAX_EDGES:
        raise ValueError(f"edges: a 1-D sequence of 2 .. {HIST_MAX_EDGES} values, got shape {e.shape}")
    if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError("edges must be finite and strictly ascending")
    return e


def build_items(offsets, lengths) -> np.ndarray:
    """The work-item table of include/mmvae_hist.h (numpy structured array, HIST_ITEM_DTYPE): segment s = elements
    offsets[s] .. offsets[s] + lengths[s] - 1, cut into items of at most HIST_ITEM_ELEMS elements, in order."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    num = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if off.size < 1 or off.size != num.size:
        raise ValueError("offsets and lengths: two sequences of the same length >= 1")
    if (num < 1).any() or (off < 0).any():
        raise ValueError("every segment has an offset >= 0 and a length >= 1")
    J = HIST_ITEM_ELEMS
    nchunk = (num + J - 1) // J
    owner = np.repeat(np.arange(off.size), nchunk)
    first = np.cumsum(nchunk) - nchunk
    k = np.arange(int(nchunk.sum())) - first[owner]
    items = np.zeros(len(owner), dtype=np.dtype(HIST_ITEM_DTYPE))
    items["offset"] = off[owner] + k * J
    items["len"] = np.minimum(num[owner] - k * J, J)
    items["segment"] = owner
    return items


class SegmentHistograms:
    """`counts` int64 [S, n_edges - 1], `stats` fp64 [S, 8] (columns HIST_STAT_NAMES, also as attributes: `.min`,
    `.sum_squares`, ...) and `edges` (numpy fp64).  The tensors stay where they were computed; `.cpu()` is the one
    synchronising copy (counts and statistics share one buffer) and is what `tensorboard_raw` works on."""

    def __init__(self, packed: torch.Tensor, n_seg: int, edges: np.ndarray):
        nb = edges.size - 1
        self._packed, self.n_seg, self.edges = packed, n_seg, edges
        self.counts = packed[:n_seg * nb].view(n_seg, nb)
        self.stats = packed[n_seg * nb:].view(torch.float64).view(n_seg, HIST_STATS)
        self._host: Optional["SegmentHistograms"] = None if packed.is_cuda else self

    def __len__(self) -> int:
        return self.n_seg

    def __getattr__(self, name):
        if name in HIST_STAT_NAMES:
            return self.stats[:, HIST_STAT_NAMES.index(name)]
        raise AttributeError(name)

    def cpu(self) -> "SegmentHistograms":
        if self._host is None:
            self._host = SegmentHistograms(self._packed.cpu(), self.n_seg, self.edges)
        return self._host

    def tensorboard_raw(self, i: int) -> Optional[dict]:
        """Segment i as the keyword arguments of `SummaryWriter.add_histogram_raw` (min, max, num, sum, sum_squares,
        bucket_limits, bucket_counts), trimmed as torch.utils.tensorboard.summary.make_histogram trims: the first to the
        last non-empty bucket, in front of them the empty bucket to their left (a prepended 0 when the first bucket is
        itself non-empty), `bucket_limits` the right edges.  None when no finite value fell into a bucket."""
        host = self.cpu()
        counts = host.counts[i].numpy()
        filled = np.flatnonzero(counts > 0)
        if filled.size == 0:
            return None
        start, end = int(filled[0]), int(filled[-1]) + 1
        trimmed = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
        limits = self.edges[start:end + 1]
        st = host.stats[i].tolist()
        return {"min": st[0], "max": st[1], "num": int(st[2]), "sum": st[3], "sum_squares": st[4],
                "bucket_limits": limits.tolist(), "bucket_counts": [int(c) for c in trimmed]}


def _pack_buffer(n_seg: int, nb: int, device) -> torch.Tensor:
    return torch.empty(n_seg * (nb + HIST_STATS), dtype=torch.int64, device=device)


def _segment_histograms_cpu(values: torch.Tensor, offsets, lengths, edges: np.ndarray, scale: float) -> SegmentHistograms:
    """The semantics, in numpy: per segment np.histogram(v.astype(float64), bins=edges) of the finite
    v = float32(values * float32(scale)) and their moments in fp64."""
    v_all = values.detach().numpy()
    S, nb = len(offsets), edges.size - 1
    packed = _pack_buffer(S, nb, "cpu")
    out = SegmentHistograms(packed, S, edges)
    counts, stats = out.counts.numpy(), out.stats.numpy()
    for s, (o, n) in enumerate(zip(offsets, lengths)):
        v = v_all[int(o):int(o) + int(n)]
        if scale != 1.0:
            v = v * np.float32(scale)
        f = v[np.isfinite(v)].astype(np.float64)
        counts[s] = np.histogram(f, bins=edges)[0]
        stats[s] = (f.min() if f.size else np.inf, f.max() if f.size else -np.inf, f.size, f.sum(), np.dot(f, f),
                    v.size - f.size, np.count_nonzero(f < edges[0]), np.count_nonzero(f > edges[-1]))
    return out


def segment_histograms(values: torch.Tensor, offsets: Sequence[int], lengths: Sequence[int], edges=None,
                       scale: float = 1.0, cache: Optional[Dict] = None) -> SegmentHistograms:
    """Histogram and moments of every segment values[offsets[s] : offsets[s] + lengths[s]] of the flat fp32 tensor
    `values`, each value multiplied by `scale` in fp32 first, over `edges` (default: tensorboard_edges()) with the
    semantics of np.histogram(v.astype(float64), bins=edges).  Segments may start anywhere and have any length >= 1.
    `cache`: a dict of the caller's that keeps the device copies of the item table and of the edges between calls with
    the same segments and edges (HipAdam.grad_histograms).  Enqueues on the current stream; nothing is synchronised."""
    if not torch.is_tensor(values) or values.dtype != torch.float32 or values.dim() != 1 or not values.is_contiguous():
        raise ValueError("values: a flat contiguous fp32 tensor")
    e = tensorboard_edges() if edges is None else check_edges(edges)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    num = np.asarray(lengths, dtype=np.int64).reshape(-1)
    items = build_items(off, num)
    if int((off + num).max()) > values.numel():
        raise ValueError("a segment reaches past the end of values")
    S, nb = off.size, e.size - 1
    if not values.is_cuda:
        return _segment_histograms_cpu(values, off, num, e, float(scale))
    lib = _hist_lib.load_hist()
    dev = values.device
    key = ("tables", dev, off.tobytes(), num.tobytes(), e.tobytes())
    tables = cache.get(key) if cache is not None else None
    if tables is None:
        items_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
        edges_dev = torch.from_numpy(e.copy()).to(dev)
        need = lib.mmvae_hist_workspace_bytes(len(items), S, e.size)
        ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
        tables = (items_dev, edges_dev, ws, len(items))
        if cache is not None:
            cache.clear()  # (one set of segments at a time: the tables of the last call)
            cache[key] = tables
    items_dev, edges_dev, ws, n_items = tables
    packed = _pack_buffer(S, nb, dev)
    out = SegmentHistograms(packed, S, e)
    rc = lib.mmvae_hist_segments_f32(n_items, items_dev.data_ptr(), S, values.data_ptr(), float(scale), e.size,
                                     edges_dev.data_ptr(), out.counts.data_ptr(), out.stats.data_ptr(), ws.data_ptr(),
                                     ws.numel() * 8, stream(dev))
    _hist_lib.check(rc, "mmvae_hist_segments_f32")
    out._keep = tables  # the tables outlive the launch
    return out
