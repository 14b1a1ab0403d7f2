"""The case lists and inputs of tests/test_fc_tails_gpu.py, shared with tests/test_fc_tails_host.py (which checks the
restatement and the cases themselves without a GPU).  Inputs are made once per case and are read-only.

Column tail: a covering list, not the product.  Every batch size, width and slab count below appears with and without
BatchNorm (test_fc_tails_host.py asserts it).  The batch sizes reach a single row, a batch inside the first 8 rows, the
chunk boundary 31 | 32 | 33, and 9, 10 and 17 chunks of 32 rows (257 / 288, 300, 513): groups of eight chunk partials
of which the last is ragged.  The slab counts run the four-slab body alone (4), the remainder alone (1) and both (5, 7, 9).
"""
import functools
from collections import namedtuple

import numpy as np

B_VALUES = (1, 2, 7, 9, 31, 32, 33, 257, 288, 300, 513)
N_VALUES = (1, 63, 64, 65, 130, 200)
S_VALUES = (1, 4, 5, 7, 9)
DATA = ("centred", "offset")
MOMENTUM, BN_EPS, LN_EPS = 0.01, 1e-3, 1e-5

ColumnCase = namedtuple("ColumnCase", "B N S_fwd S_bwd bn bias affine running nbt relu p addend addend_a row_scale")


def _column_cases():
    cases = []
    for bn in (True, False):
        for i in range(22):
            B = B_VALUES[i % 11]
            N = N_VALUES[(i + 2 * (i // 11) + (0 if bn else 3)) % 6]
            # options: every one is on and off with and without BatchNorm.  A case never has both one slab and no bias
            # (forward), or one slab and nothing that rounds (backward): its outputs would be exact copies of its inputs
            # and say nothing about arithmetic.  Column 0 of the offset data is negative: no ReLU over it without BatchNorm.
            cases.append(ColumnCase(
                B=B, N=N, S_fwd=S_VALUES[i % 5], S_bwd=S_VALUES[(3 * i + 1) % 5], bn=bn,
                bias=i % 3 != 0 or i % 5 == 0, affine=i % 4 != 2, running=i % 5 != 4, nbt=i % 5 != 4 and i % 2 == 0,
                relu=i % 4 != 3 and (bn or N != 1), p=0.25 if i % 3 == 1 else 0.0, addend=i % 2 == 1 or i == 18,
                addend_a=i % 4 in (0, 1), row_scale=i % 3 == 2))
    return tuple(cases)


COLUMN_CASES = _column_cases()
# eval mode (running statistics): a BatchNorm case of every chunk count class, each with and without a mask
EVAL_CASES = tuple(c for c in COLUMN_CASES if c.bn and c.running and c.B in (1, 9, 33, 257, 513))
PLANE_SHAPES = ((33, 130), (300, 66))  # N even and off a multiple of 64

RowCase = namedtuple("RowCase", "rows N S_fwd S_bwd bias relu p addend row_scale deferred")
# rows: one wave of a block, a ragged last block of four rows (5, 33), two chunks of 32 (33).  N: a single column, the
# wave width and the register classes' boundaries 256 | 512 | 513, 768 | 769, and 1025 beyond the widest class.
ROW_CASES = (
    RowCase(1, 1, 1, 3, True, True, 0.0, False, False, False),
    RowCase(5, 1, 3, 1, False, False, 0.0, True, True, True),
    RowCase(5, 64, 3, 1, False, True, 0.25, True, False, False),
    RowCase(33, 65, 1, 3, True, False, 0.25, False, True, True),
    RowCase(1, 256, 3, 3, True, True, 0.0, True, True, False),
    RowCase(5, 512, 1, 1, True, True, 0.25, True, False, True),
    RowCase(33, 513, 3, 1, True, True, 0.0, False, True, False),
    RowCase(1, 768, 1, 3, False, False, 0.25, True, False, False),
    RowCase(5, 769, 3, 3, True, True, 0.0, True, True, True),
    RowCase(33, 1025, 1, 3, True, True, 0.25, True, False, False),
    RowCase(33, 1025, 3, 1, False, True, 0.0, False, True, True),
    RowCase(33, 768, 1, 1, True, True, 0.25, True, True, True),
)
LN_CASES = tuple((B, N) for B in (1, 3, 5) for N in (1, 63, 64, 65))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def column_means_and_stds(N):
    """the "offset" data: column c has mean 100 ((c mod 3) - 1) + 30 and std 0.1 (even c) or 1 (odd c)"""
    c = np.arange(N)
    return 100.0 * ((c % 3) - 1) + 30.0, np.where(c % 2 == 0, 0.1, 1.0)


@functools.lru_cache(maxsize=None)
def column_inputs(case, data):
    """fp32 inputs of one column case: slabs [S_fwd, B, N] whose sum is the data set, the BatchNorm vectors, the keep
    mask, and the backward pass's gradient slabs, addends and row weights (centred in both data sets)."""
    B, N = case.B, case.N
    rng = np.random.default_rng([COLUMN_CASES.index(case), DATA.index(data), 2024])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    if data == "offset":
        mu, sd = column_means_and_stds(N)
    else:
        mu, sd = np.zeros(N), np.ones(N)
    target = mu + sd * rng.standard_normal((B, N))
    slabs = f32(0.5 * sd * rng.standard_normal((case.S_fwd, B, N)))
    slabs[0] = f32(target - slabs[1:].astype(np.float64).sum(0))
    inp = dict(
        slabs=slabs, bias=f32(0.1 * rng.standard_normal(N)),
        gamma=f32(1 + 0.1 * rng.standard_normal(N)), beta=f32(0.1 * rng.standard_normal(N)),
        # running statistics near the data's, so that eval mode normalises to O(1) values
        running_mean=f32(mu + 0.1 * sd * rng.standard_normal(N)),
        running_var=f32(sd * sd * (1 + 0.1 * np.abs(rng.standard_normal(N)))),
        mask=(rng.random((B, N)) >= 0.25).astype(np.uint8),
        din=f32(rng.standard_normal((case.S_bwd, B, N))), addend=f32(rng.standard_normal((B, N))),
        addend_a=f32(rng.standard_normal((B, N))), row_scale=f32(rng.random(B) + 0.5))
    return _frozen(inp)


def column_bn(case, inp):
    """the `bn` dict of the restatement for a case (None without BatchNorm)"""
    if not case.bn:
        return None
    return dict(gamma=inp["gamma"] if case.affine else None, beta=inp["beta"] if case.affine else None,
                running_mean=inp["running_mean"] if case.running else None,
                running_var=inp["running_var"] if case.running else None, momentum=MOMENTUM, eps=BN_EPS)


@functools.lru_cache(maxsize=None)
def row_inputs(case):
    rows, N = case.rows, case.N
    rng = np.random.default_rng([ROW_CASES.index(case), 77])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return _frozen(dict(
        slabs=f32(rng.standard_normal((case.S_fwd, rows, N))), bias=f32(0.3 * rng.standard_normal(N)),
        mask=(rng.random((rows, N)) >= 0.25).astype(np.uint8), din=f32(rng.standard_normal((case.S_bwd, rows, N))),
        addend=f32(rng.standard_normal((rows, N))), row_scale=f32(rng.random(rows) + 0.5)))


@functools.lru_cache(maxsize=None)
def ln_inputs(B, N):
    rng = np.random.default_rng([B, N, 5])
    return _frozen(dict(x=np.float32(rng.standard_normal((B, N)) + 0.5), g=np.float32(rng.standard_normal((B, N)))))
