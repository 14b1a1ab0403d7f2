"""Raw counts -> what the model trains on: the reference's `normalize_data` and `get_data_stats`
(scripts/data-preprocessing/data_processing_functions.py:12-51) for a whole CSR chunk at once.

`normalize_csr_` rewrites a `torch.sparse_csr_tensor` of raw counts in place, row by row:

    s = fl32(sum of the row's stored values)           (accumulated in fp64, rounded once)
    v <- log1p( fl32( fl32(v * target_sum) / s ) )     (fp32 multiply, then a true fp32 division, then log1p in fp32)

which is the reference's `np.log1p((row_data * 1e4) / row_data.sum())` -- bit for bit on the host for counts whose row
total stays below 2^24 (tests/golden/prep_normalize.npz).  Device tensors go through libmmvae_prep.so
(include/mmvae_prep.h: one launch, a wave per row) -- missing, it raises: no torch fallback.  CPU tensors go through numpy
(`_normalize_cpu`): the host tests and CPU feeds run on it, and it states the arithmetic.  The two agree on the row sums
exactly and on every element to the last bits of fp32 (either lies within 5e-7 relative of an fp64 evaluation; the
log1p of the device is its own, within 2 ulp).

Deviation from the reference: a row whose stored values sum to 0 (stored zeros) gets 0.0 in every element.  The reference
divides 0 by 0 there and writes NaN under numpy's "invalid value" warning.

`RowSumStats` accumulates the per-cell totals the normalisation hands out into the mean and standard deviation that the
reference's census_data_stats.py records per chunk file.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import numpy as np
import torch

NORMALIZE_MODES = ("log1p_cpm",)


def check_target_sum(target_sum: float) -> float:
    t = float(target_sum)
    f32 = np.finfo(np.float32)
    if not math.isfinite(t) or not float(f32.tiny) <= t <= float(f32.max):  # (the kernel takes it as fp32)
        raise ValueError(f"target_sum must be finite and positive, got {target_sum!r}")
    return t


def _normalize_cpu(crow: np.ndarray, values: np.ndarray, target_sum: float) -> np.ndarray:
    """The arithmetic, stated in numpy on a host CSR: `values` (fp32, writable) in place; returns the fp32 row sums."""
    n = len(crow) - 1
    start = np.asarray(crow[:-1], dtype=np.int64)
    length = np.asarray(crow[1:], dtype=np.int64) - start
    nz = np.flatnonzero(length > 0)
    sums64 = np.zeros(n, dtype=np.float64)
    lo, hi = int(crow[0]), int(crow[-1])
    if nz.size:  # (reduceat needs strictly valid starts: the non-empty rows tile [lo, hi) without gaps)
        sums64[nz] = np.add.reduceat(values[lo:hi].astype(np.float64), start[nz] - lo)
    sums = sums64.astype(np.float32)
    per_elem = np.repeat(sums, length)
    t = np.float32(target_sum)
    seg = values[lo:hi]
    dead = per_elem == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.log1p((seg * t) / per_elem).astype(np.float32, copy=False)
    out[dead] = 0.0
    seg[...] = out
    return sums


def normalize_csr_(csr: torch.Tensor, target_sum: float = 1e4,
                   return_row_sums: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """Normalise the raw counts of a 2-D `torch.sparse_csr_tensor` (fp32 values, int32 or int64 indices) IN PLACE and
    return it -- with `return_row_sums`, `(csr, row_sums)`: the fp32 totals of the raw rows, on the tensor's device.  On a
    device tensor the work is enqueued on the current stream and nothing is synchronised."""
    if not torch.is_tensor(csr) or csr.layout != torch.sparse_csr or csr.dim() != 2:
        raise ValueError("normalize_csr_: expected a 2-D torch.sparse_csr tensor")
    crow, values = csr.crow_indices(), csr.values()
    if values.dtype != torch.float32:
        raise TypeError(f"normalize_csr_: expected fp32 values, got {values.dtype}")
    if crow.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"normalize_csr_: expected int32 or int64 indices, got {crow.dtype}")
    t = check_target_sum(target_sum)
    n_rows = int(csr.shape[0])
    if n_rows < 1:
        row_sums = torch.zeros(0, dtype=torch.float32, device=values.device)
    elif values.is_cuda:
        from . import ops

        if not (crow.is_contiguous() and values.is_contiguous()):
            raise ValueError("normalize_csr_: the tensor's arrays must be contiguous")
        row_sums = torch.empty(n_rows, dtype=torch.float32, device=values.device) if return_row_sums else None
        ops.csr_log1p_normalize_(crow, values, t, row_sums)
    else:
        if not values.is_contiguous():
            raise ValueError("normalize_csr_: the tensor's arrays must be contiguous")
        row_sums = torch.from_numpy(_normalize_cpu(crow.numpy(), values.numpy(), t))
    return (csr, row_sums) if return_row_sums else csr


class RowSumStats:
    """Accumulator of (n, sum s, sum s^2) over the per-cell totals `row_sums`, one chunk at a time, in fp64 / Python
    floats.  `.mean` and `.std` (population, ddof = 0) are the reference's `get_data_stats` -- of one chunk when fed one
    chunk, of the whole data set when fed every chunk.  On a device tensor a chunk costs two fp64 reductions."""

    def __init__(self):
        self.n, self.sum, self.sum_squares = 0, 0.0, 0.0

    def update(self, row_sums) -> "RowSumStats":
        s = torch.as_tensor(row_sums).reshape(-1).to(torch.float64)
        if s.numel():
            self.n += int(s.numel())
            self.sum += float(s.sum())
            self.sum_squares += float((s * s).sum())
        return self

    @property
    def mean(self) -> float:
        return self.sum / self.n if self.n else float("nan")

    @property
    def std(self) -> float:
        if not self.n:
            return float("nan")
        m = self.sum / self.n
        return math.sqrt(max(self.sum_squares / self.n - m * m, 0.0))

    @classmethod
    def of(cls, row_sums) -> "RowSumStats":
        return cls().update(row_sums)
