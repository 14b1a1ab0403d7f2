"""The case lists and inputs of tests/test_cond_layers_gpu.py, shared with tests/test_cond_layers_host.py (which checks the
restatement, the bound and the coverage of these lists without a GPU).  Inputs are made once per case and are read-only.

A covering list, not a product: tests/test_cond_layers_host.py asserts which classes of csrc/cond_layers.hip it reaches.

Data.  "exact": W, x, dy, the bias and the old dx are integers in [-3, 3] -- every product and every sum is exact in float32,
so the device must reproduce the fp64 restatement bit for bit; "random": normal entries, the weights scaled by 0.3.

Arena.  The blocks of all positions lie in one arena in shuffled order, all weights first, then all biases in another
order (a block's weight and bias are never adjacent); the gap in front of the i-th placed tensor is i mod 4 floats (plus 4
now and then), so weight offsets of every residue mod 4 occur; gaps hold the sentinel NaN.  Some blocks of every bank are
absent from the batch.

Label layouts.  "one": all cells in one block; "distinct": every cell its own block; "runs": blocks of 1, 31, 32, 33, 64,
65, 128, 129, 161 and 257 cells in one batch of 901 with shuffled labels (34 chunks of at most 32 cells, piece counts 2,
2, 3, 4, 5, 6, 9); "mixed": random labels."""
import functools
from collections import namedtuple

import numpy as np

from mmvae_amd import cond_tables as CT

SENT = 0x7FC0BEEF  # the NaN bit pattern of tests/test_fc_tails_gpu.py
RUN_COUNTS = (1, 31, 32, 33, 64, 65, 128, 129, 161, 257)
B_VALUES = (1, 7, 8, 9, 33, 901)
LAYOUTS = ("one", "distinct", "runs", "mixed")
DATA = ("exact", "random")

# wide: every leading dimension of the call lies above its width (sentinel slack)
FwdCase = namedtuple("FwdCase", "n_in n_out B layout data wide")
DxCase = namedtuple("DxCase", "n_in n_out B layout data n_pos wide")
DwCase = namedtuple("DwCase", "n_out n_in B layout data padded wide")

FWD_SHAPES = ((1, 1, 901, "runs"), (63, 5, 7, "mixed"), (64, 4, 8, "one"), (65, 17, 9, "distinct"), (128, 128, 33, "mixed"),
              (129, 3, 1, "one"), (192, 16, 33, "distinct"), (193, 9, 901, "runs"), (256, 31, 9, "mixed"),
              (257, 3, 8, "distinct"), (8192, 3, 7, "mixed"))
FWD_CASES = tuple(FwdCase(n_in, n_out, B, lay, data, (i + d) % 2 == 0)
                  for i, (n_in, n_out, B, lay) in enumerate(FWD_SHAPES) for d, data in enumerate(DATA))
FWD_N_POS = 3       # positions of a forward case with n_in <= 256 (mmvae_cond_linear_fwd_multi runs 1 and 3 of them)

# n_pos: positions of mmvae_cond_linear_bwd_dx_multi (refused beyond n_out = 1024: the case then has one position)
DX_SHAPES = ((1, 1, 9, "mixed", 6), (127, 7, 8, "one", 2), (128, 15, 33, "distinct", 1), (129, 16, 901, "runs", 2),
             (257, 17, 7, "mixed", 6), (128, 129, 33, "mixed", 2), (5, 1024, 9, "distinct", 2), (3, 1025, 8, "mixed", 1),
             (5, 8192, 1, "one", 1), (3, 8192, 7, "mixed", 1))
DX_CASES = tuple(DxCase(n_in, n_out, B, lay, data, n_pos, (i + d) % 2 == 1)
                 for i, (n_in, n_out, B, lay, n_pos) in enumerate(DX_SHAPES) for d, data in enumerate(DATA))

DW_SHAPES = ((1, 1, 7, "one"), (8, 200, 33, "mixed"), (128, 128, 9, "distinct"), (129, 127, 33, "one"),
             (130, 260, 8, "mixed"), (70, 130, 901, "runs"), (7, 9, 901, "runs"), (8, 200, 1, "one"))
DW_CASES = tuple(DwCase(n_out, n_in, B, lay, data, (i + d) % 2 == 0, (i // 2 + d) % 2 == 0)
                 for i, (n_out, n_in, B, lay) in enumerate(DW_SHAPES) for d, data in enumerate(DATA))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def values(rng, data, shape, scale=1.0):
    if data == "exact":
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def labels(rng, layout, B):
    """-> (block index of every cell inside its bank [B] int32, blocks of the bank); at least two blocks stay absent"""
    if layout == "one":
        return np.full(B, 1, np.int32), 3
    if layout == "distinct":
        return rng.permutation(B + 2)[:B].astype(np.int32), B + 2
    if layout == "runs":
        assert B == sum(RUN_COUNTS)
        ids = rng.permutation(len(RUN_COUNTS) + 3)[:len(RUN_COUNTS)]
        return rng.permutation(np.repeat(ids, RUN_COUNTS)).astype(np.int32), len(RUN_COUNTS) + 3
    assert layout == "mixed"
    n = max(4, min(B // 3 + 3, 16))
    ids = rng.permutation(n)[:n - 2]
    return ids[rng.integers(0, n - 2, B)].astype(np.int32), n


def offsets_only(rng, n_blocks, n_out, n_in):
    """-> (w_off, b_off int64 [n_blocks], floats of the arena): the layout described above"""
    order_w, order_b = rng.permutation(n_blocks), rng.permutation(n_blocks)
    if order_w[-1] == order_b[0]:
        order_b = np.roll(order_b, 1)
    w_off, b_off = np.zeros(n_blocks, np.int64), np.zeros(n_blocks, np.int64)
    pos, i = 5, 0
    for off, order, size in ((w_off, order_w, n_out * n_in), (b_off, order_b, n_out)):
        for c in order:
            pos += i % 4 + (4 if i % 5 == 2 else 0)
            off[c] = pos
            pos += size
            i += 1
    return w_off, b_off, pos + 3


def make_arena(rng, data, n_blocks, n_out, n_in):
    """-> (arena float32 with the sentinel in its gaps, w_off, b_off)"""
    w_off, b_off, size = offsets_only(rng, n_blocks, n_out, n_in)
    arena = np.full(size, SENT, np.uint32).view(np.float32)
    for c in range(n_blocks):
        arena[w_off[c]:w_off[c] + n_out * n_in] = values(rng, data, n_out * n_in, 0.3)
        arena[b_off[c]:b_off[c] + n_out] = values(rng, data, n_out)
    return arena, w_off, b_off


def banks(rng, layouts, B):
    """labels of several positions, each with a bank of its own -> (cond [n_pos, B] global block indices, bases, blocks)"""
    cond, bases, total = [], [], 0
    for lay in layouts:
        local, n = labels(rng, lay, B)
        cond.append(local + total)
        bases.append(total)
        total += n
    return np.stack(cond).astype(np.int32), bases, total


def other_layouts(case, n_pos):
    """position 0 has the case's layout, the others "mixed" and "distinct" in turn ("one" in place of "distinct" for a
    single cell and for the large batch, whose 901 blocks would fill megabytes)"""
    more = ("mixed", "distinct") if 1 < case.B < 100 else ("mixed", "one")
    return (case.layout,) + tuple(more[j % 2] for j in range(n_pos - 1))


@functools.lru_cache(maxsize=None)
def fwd_inputs(case):
    rng = np.random.default_rng([FWD_CASES.index(case), 11])
    n_pos = FWD_N_POS if case.n_in <= 256 else 1
    cond, bases, total = banks(rng, other_layouts(case, n_pos), case.B)
    arena, w_off, b_off = make_arena(rng, case.data, total, case.n_out, case.n_in)
    return _frozen(dict(cond=cond, arena=arena, w_off=w_off, b_off=b_off,
                        x=values(rng, case.data, (n_pos, case.B, case.n_in))))


@functools.lru_cache(maxsize=None)
def dx_inputs(case):
    rng = np.random.default_rng([DX_CASES.index(case), 12])
    cond, bases, total = banks(rng, other_layouts(case, case.n_pos), case.B)
    arena, w_off, _ = make_arena(rng, case.data, total, case.n_out, case.n_in)
    return _frozen(dict(cond=cond, arena=arena, w_off=w_off, dy=values(rng, case.data, (case.n_pos, case.B, case.n_out)),
                        old=values(rng, case.data, (case.B, case.n_in))))


@functools.lru_cache(maxsize=None)
def dw_inputs(case):
    rng = np.random.default_rng([DW_CASES.index(case), 13])
    cond, bases, total = banks(rng, (case.layout,), case.B)
    w_off, b_off, size = offsets_only(rng, total, case.n_out, case.n_in)
    return _frozen(dict(cond=cond[0], w_off=w_off, b_off=b_off, size=size, dy=values(rng, case.data, (case.B, case.n_out)),
                        x=values(rng, case.data, (case.B, case.n_in))))


MultiDw = namedtuple("MultiDw", "form n_pos R Z data")
# the two forms in which the engine calls mmvae_cond_linear_bwd_dw_multi (engine_cond.py, emit_backward)
MULTI_DW = tuple(MultiDw(form, 4, 70, 24, data) for form in ("deferred", "parallel") for data in DATA)


@functools.lru_cache(maxsize=None)
def multi_dw_inputs(case):
    """n_pos positions of R cells and width Z.  "deferred" (sequential order): x [n_pos, R, Z] holds every position's own
    input, dy [n_pos, R, Z]; the engine's batched launch covers positions 1 .. n_pos - 1.  "parallel": one x [R, Z] for all
    positions, dy [n_pos, R, Z] are the column blocks of one wide matrix.  Position 1 has one block for all cells (three
    pieces), the others mixed and distinct labels."""
    rng = np.random.default_rng([MULTI_DW.index(case), 14])
    layouts = ("mixed", "one", "distinct", "mixed")[:case.n_pos]
    cond, bases, total = banks(rng, layouts, case.R)
    w_off, b_off, size = offsets_only(rng, total, case.Z, case.Z)
    x_shape = (case.n_pos, case.R, case.Z) if case.form == "deferred" else (case.R, case.Z)
    return _frozen(dict(cond=cond, w_off=w_off, b_off=b_off, size=size, dy=values(rng, case.data, (case.n_pos, case.R, case.Z)),
                        x=values(rng, case.data, x_shape)))


def tables(cond, padded=False):
    """cond_tables.group_tables of one position's global block indices; padded: the fixed-size form of a captured program
    (chunk and reduction lists filled up to their maxima with -1)"""
    t = CT.group_tables(np.asarray(cond, np.int32))
    if padded:
        R = len(cond)
        seg = np.zeros(CT.words(R), np.int32)
        CT.fill_padded(seg, t, R)
        lay = CT.layout(R)
        sizes = dict(cond=R, rows=R, chunk_dst=CT.max_chunks(R), chunk_beg=CT.max_chunks(R), chunk_end=CT.max_chunks(R),
                     red_cond=CT.max_reductions(R), red_slot=CT.max_reductions(R), red_n=CT.max_reductions(R))
        t = dict({k: seg[lay[k]:lay[k] + n].copy() for k, n in sizes.items()}, present=t["present"])
    return t
