"""The conditional-layer kernels of mmvae_amd/csrc/cond_layers.hip against the fp64 restatement (tests/cond_restatement.py,
itself held to a per-condition torch loop with autograd in tests/test_cond_layers_host.py): mmvae_cond_linear_fwd,
_bwd_dx, _bwd_dw and their _multi forms, called through ctypes so that every argument is free -- leading dimensions above
the width, position strides, table strides, NULL options, refusals.  The cases (tests/cond_cases.py; what they reach is
asserted in the host file) run every instantiation T = 1 .. 4 of the sorted forward and both sides of 64 | 65, 128 | 129,
192 | 193 and 256 | 257, the maxima 8192; for dx odd and tiny n_out, one to three passes of 128 input columns, 1024 | 1025;
for dW one to six tiles, every n_in mod 4, weight offsets of every residue mod 4 (16-byte and element stores), chunks of
1, 31 and 32 cells, 2 .. 6 and 9 partial pieces, exact and padded tables.

Buffers.  Every output lies in a buffer with slack columns up to its leading dimension and sentinel rows before and
behind it, all filled with one NaN bit pattern, which must be there after every call; inputs and the parameter arena carry
the same NaN in their slack and gaps.  The gradient arena is sentinel-filled: after dW the present blocks hold the values
(written, not accumulated), absent blocks and all gaps still the sentinel.  The scratch slots are filled before every call,
once with the sentinel and once with large finite values: the result does not depend on them.

Bounds (derived, not measured).  On the "exact" data (small integers) the device equals the fp64 restatement bit for bit
(a zero of the restatement taken as +0: a sum that starts at +0 never gives -0).  On the "random" data, per element,
|device - fp64| <= (n + 3) 2^-24 S: n the number of products summed into the element (n_in for y; n_pos n_out, + 1 with
accumulate, for dx; the block's cell count for dW and db), S the same sum over absolute values (cond_restatement.py).
That is the standard bound of a float32 sum of n products in any order, with or without contraction; + 3 covers the bias,
the addition of the two half-sums and the factor 1 / (1 - n u).  Each test prints the largest ratio of deviation to bound
it saw; the largest per entry are in profiles/cond_layers.txt.

Bit-for-bit properties, each stated in the kernel comments: sorted forward == one-cell forward; _fwd_multi == one _fwd
per position; _bwd_dw_multi == one _bwd_dw per position in both layouts of the engine; two dW calls are equal; a block's dW
and db do not depend on the other blocks' cells; the sorted dx of a cell does not depend on how its set is grouped.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mmvae_amd import cond_tables as CT
from tests import cond_cases as CC
from tests import cond_restatement as R
from tests.test_fc_tails_gpu import SENT, Mat, Vec

pytestmark = pytest.mark.gpu
assert SENT == CC.SENT

MAXIMA = {}  # entry -> largest deviation / bound

ARGS = {
    "mmvae_cond_linear_fwd": "B n_in n_out x ldx params w_off b_off cond rows y ldy stream",
    "mmvae_cond_linear_bwd_dx": "B n_in n_out dy lddy params w_off cond rows dx lddx accumulate stream",
    "mmvae_cond_linear_bwd_dw": "n_chunks chunk_dst chunk_beg chunk_end rows n_in n_out dy lddy x ldx grads w_off b_off "
                                "n_red red_cond red_slot red_n partials stream",
    "mmvae_cond_linear_fwd_multi": "n_pos B n_in n_out x ldx x_pos_stride params w_off b_off cond rows tbl_stride y ldy "
                                   "y_pos_stride stream",
    "mmvae_cond_linear_bwd_dx_multi": "n_pos B n_in n_out dy lddy dy_pos_stride params w_off cond tbl_stride dx lddx "
                                      "accumulate stream",
    "mmvae_cond_linear_bwd_dw_multi": "n_pos n_chunks chunk_dst chunk_beg chunk_end rows tbl_stride n_in n_out dy lddy "
                                      "dy_pos_stride x ldx x_pos_stride grads w_off b_off n_red red_cond red_slot red_n "
                                      "partials part_pos_stride stream",
}
FWD, DX, DW = "mmvae_cond_linear_fwd", "mmvae_cond_linear_bwd_dx", "mmvae_cond_linear_bwd_dw"


def call(name, **kw):
    """One C entry by keyword; what is not given is NULL / 0.  Buffers are passed as themselves, tensors by their
    address, an address as an integer."""
    from mmvae_amd import _lib

    lib = _lib.load()
    names, types = ARGS[name].split(), _lib.PROTOTYPES[name][1]
    assert len(names) == len(types) and not set(kw) - set(names), set(kw) - set(names)
    args = []
    for n, t in zip(names, types):
        v = kw.get(n)
        if n == "stream":
            v = torch.cuda.current_stream().cuda_stream
        elif hasattr(v, "ptr"):
            v = v.ptr()
        elif torch.is_tensor(v):
            v = v.data_ptr()
        elif v is None and t in (C.c_int, C.c_int64):
            v = 0
        args.append(v)
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    return rc


def dev(a):
    """a host array on the device, bit for bit (sentinels in gaps included)"""
    return torch.from_numpy(np.array(a)).cuda()


def blocks_in_columns(a, stride):
    """[n_pos, B, w] -> float32 [B, (n_pos - 1) stride + w]: position j in columns j stride .., the sentinel between"""
    n_pos, B, w = a.shape
    out = np.full((B, (n_pos - 1) * stride + w), SENT, np.uint32).view(np.float32)
    for j in range(n_pos):
        out[:, j * stride:j * stride + w] = a[j]
    return out


def held(entry, case, got, want, n, S):
    """exact data: equal bits; random data: per element |got - want| <= (n + 3) 2^-24 S.  NaN in `want`: no value there."""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.dtype == np.float32 and got.shape == want.shape
    ok = ~np.isnan(want)
    assert np.isfinite(got[ok]).all(), entry
    if case.data == "exact":
        assert np.array_equal(got[ok].view(np.uint32), (want[ok] + 0.0).astype(np.float32).view(np.uint32)), entry
        return
    lim = R.bound(n[ok] if np.ndim(n) else n, S[ok])
    dev_ = np.abs(got[ok].astype(np.float64) - want[ok])
    ratio = float((dev_ / np.where(lim > 0, lim, 1.0)).max())
    print(f"  {entry}: largest deviation / bound {ratio:.3f}")
    MAXIMA[entry] = max(MAXIMA.get(entry, 0.0), ratio)
    assert (dev_ <= lim).all(), (entry, ratio)


@pytest.fixture(scope="module", autouse=True)
def summary():
    MAXIMA.clear()
    yield
    print("\nlargest deviation from the fp64 restatement over its bound (n + 3) 2^-24 S, per entry and path:")
    for entry, ratio in sorted(MAXIMA.items()):
        print(f"cond-layers-summary {entry:44s} {ratio:.3f}")


def table_pack(arrays, stride):
    """int32 [n_pos, stride]: position j's arrays one behind the other -> (device tensor, {name: address at position 0})"""
    n_pos = len(arrays)
    pack = np.zeros((n_pos, stride), np.int32)
    offs, o = {}, 0
    for name in arrays[0]:
        width = max(len(a[name]) for a in arrays)
        for j, a in enumerate(arrays):
            pack[j, o:o + len(a[name])] = a[name]
        offs[name] = o
        o += width
    assert o <= stride
    t = dev(pack)
    return t, {name: t.data_ptr() + 4 * o for name, o in offs.items()}


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", CC.FWD_CASES, ids=lambda c: f"{c.n_in}x{c.n_out}-{c.B}-{c.layout}-{c.data}")
def test_forward_one_cell_sorted_and_multi(case):
    print(f"\n{case}")
    inp = CC.fwd_inputs(case)
    B, n_in, n_out, cond = case.B, case.n_in, case.n_out, inp["cond"]
    n_pos = cond.shape[0]
    ldx, ldy = n_in + (3 if case.wide else 0), n_out + (5 if case.wide else 0)
    params, wo, bo = dev(inp["arena"]), dev(inp["w_off"]), dev(inp["b_off"])
    X = Mat(n_pos * B, n_in, ldx, inp["x"])        # position j: rows j B ..
    x_at = lambda j: X.ptr() + 4 * j * B * ldx     # noqa: E731
    tabs = [CC.tables(c) for c in cond]
    stride = 2 * B + 3
    tbl, at = table_pack([dict(cond=c, rows=t["rows"]) for c, t in zip(cond, tabs)], stride)
    own = R.forward(inp["x"], inp["arena"], inp["w_off"], inp["b_off"], cond, n_out)      # every position its own input
    shared = R.forward(inp["x"][0], inp["arena"], inp["w_off"], inp["b_off"], cond, n_out)  # all read position 0's

    def single(x, j, rows):
        y = Mat(B, n_out, ldy)
        assert call(FWD, B=B, n_in=n_in, n_out=n_out, x=x, ldx=ldx, params=params, w_off=wo, b_off=bo,
                    cond=at["cond"] + 4 * j * stride, rows=at["rows"] + 4 * j * stride if rows else None, y=y, ldy=ldy) == 0
        assert y.slack_untouched()
        return y

    plain, by_rows = single(x_at(0), 0, False), single(x_at(0), 0, True)
    held("fwd one-cell", case, plain.get(), own[0][0], n_in, own[1][0])
    held("fwd sorted" if n_in <= 256 else "fwd one-cell", case, by_rows.get(), own[0][0], n_in, own[1][0])
    # the same arithmetic per output on both kernels; beyond n_in = 256 `rows` is ignored
    assert np.array_equal(by_rows.bits(), plain.bits())
    if n_in > 256:
        return
    ys = n_out + (2 if case.wide else 0)           # y_pos_stride
    for n, strided in ((1, True), (3, False), (3, True)):
        want, S = own if strided else shared
        cols = (n - 1) * ys + n_out
        y = Mat(B, cols, cols + (5 if case.wide else 0))
        assert call("mmvae_cond_linear_fwd_multi", n_pos=n, B=B, n_in=n_in, n_out=n_out, x=X, ldx=ldx,
                    x_pos_stride=B * ldx if strided else 0, params=params, w_off=wo, b_off=bo, cond=at["cond"],
                    rows=at["rows"], tbl_stride=stride, y=y, ldy=y.ld, y_pos_stride=ys) == 0
        assert y.slack_untouched()
        got = y.bits()
        for j in range(n):
            block = got[:, j * ys:j * ys + n_out]
            held("fwd_multi", case, block.view(np.float32), want[j], n_in, S[j])
            assert np.array_equal(block, single(x_at(j if strided else 0), j, True).bits())  # == one _fwd per position
            assert (got[:, j * ys + n_out:(j + 1) * ys] == SENT).all()                       # between the column blocks


# ------------------------------------------------------------------------------------------------------------------ dx
@pytest.mark.parametrize("case", CC.DX_CASES, ids=lambda c: f"{c.n_in}x{c.n_out}-{c.B}-{c.layout}-p{c.n_pos}-{c.data}")
def test_dx_one_cell_sorted_and_multi(case):
    print(f"\n{case}")
    inp = CC.dx_inputs(case)
    B, n_in, n_out, cond, n_pos = case.B, case.n_in, case.n_out, inp["cond"], case.n_pos
    ds = n_out + (1 if case.wide else 0)           # dy_pos_stride: position j's dy in columns j ds ..
    dy_host = blocks_in_columns(inp["dy"], ds)
    lddy, lddx = dy_host.shape[1] + (4 if case.wide else 0), n_in + (3 if case.wide else 0)
    DY = Mat(B, dy_host.shape[1], lddy, dy_host)
    params, wo = dev(inp["arena"]), dev(inp["w_off"])
    tabs = [CC.tables(c) for c in cond]
    stride = 2 * B + 1
    tbl, at = table_pack([dict(cond=c, rows=t["rows"]) for c, t in zip(cond, tabs)], stride)
    def single(j, rows, dx, accumulate):
        assert call(DX, B=B, n_in=n_in, n_out=n_out, dy=DY.ptr() + 4 * j * ds, lddy=lddy, params=params, w_off=wo,
                    cond=at["cond"] + 4 * j * stride, rows=at["rows"] + 4 * j * stride if rows else None, dx=dx, lddx=lddx,
                    accumulate=accumulate) == 0
        assert dx.slack_untouched()
        return dx

    for acc in (0, 1):
        old = inp["old"] if acc else None          # without accumulate the output holds the sentinel before the call
        want, S = R.input_grad(inp["dy"][:1], inp["arena"], inp["w_off"], cond[:1], n_in, old)
        plain, by_rows = single(0, False, Mat(B, n_in, lddx, old), acc), single(0, True, Mat(B, n_in, lddx, old), acc)
        held(f"bwd_dx one-cell acc={acc}", case, plain.get(), want, n_out + acc, S)
        if n_out > 1024:  # `rows` is ignored
            assert np.array_equal(by_rows.bits(), plain.bits())
            continue
        held(f"bwd_dx sorted acc={acc}", case, by_rows.get(), want, n_out + acc, S)
        for n in sorted({1, n_pos}):
            want, S = R.input_grad(inp["dy"][:n], inp["arena"], inp["w_off"], cond[:n], n_in, old)
            dx = Mat(B, n_in, lddx, old)
            assert call("mmvae_cond_linear_bwd_dx_multi", n_pos=n, B=B, n_in=n_in, n_out=n_out, dy=DY, lddy=lddy,
                        dy_pos_stride=ds, params=params, w_off=wo, cond=at["cond"], tbl_stride=stride, dx=dx, lddx=lddx,
                        accumulate=acc) == 0
            assert dx.slack_untouched()
            held(f"bwd_dx_multi acc={acc}", case, dx.get(), want, n * n_out + acc, S)
        if n_pos > 1:
            # one sorted launch per position, in descending order as the engine issues them: the same bound (no bits promised)
            chain = Mat(B, n_in, lddx, old)
            for j in range(n_pos - 1, -1, -1):
                single(j, True, chain, acc if j == n_pos - 1 else 1)
            held(f"bwd_dx sorted, per position acc={acc}", case, chain.get(), want, n_pos * n_out + acc, S)


def test_sorted_dx_of_a_cell_does_not_depend_on_the_grouping_of_its_set():
    """cond_linear_bwd_dx_sorted_kernel: a set of eight sorted cells that share one block is computed by one workgroup (all
    eight per loaded weight), otherwise one workgroup per cell; per cell the arithmetic is the same.  Eleven cells: a full set
    and a ragged one; the same cell, dy row and weights on both paths."""
    B, n_in, n_out = 11, 129, 17
    rng = np.random.default_rng(17)
    arena, w_off, _ = CC.make_arena(rng, "random", B + 1, n_out, n_in)
    dy = CC.values(rng, "random", (B, n_out))
    DY, params, wo = Mat(B, n_out, n_out + 2, dy), dev(arena), dev(w_off)

    def run(cond):
        cond = np.asarray(cond, np.int32)
        dx = Mat(B, n_in, n_in + 1)
        assert call(DX, B=B, n_in=n_in, n_out=n_out, dy=DY, lddy=n_out + 2, params=params, w_off=wo, cond=dev(cond),
                    rows=dev(CT.group_tables(cond)["rows"]), dx=dx, lddx=n_in + 1) == 0
        assert dx.slack_untouched()
        return dx.bits()

    together = run(np.full(B, B))                    # sorted order = batch order: sets {0 .. 7} and {8, 9, 10}
    for cell in (0, 5, 7, 9):
        cond = np.arange(B)
        cond[cell] = B                               # sorted last: alone in its workgroup, the set is not uniform
        assert np.array_equal(run(cond)[cell], together[cell]), cell
    want, S = R.input_grad(dy, arena, w_off, np.full(B, B), n_in)
    assert (np.abs(together.view(np.float32) - want) <= R.bound(n_out, S)).all()


# ------------------------------------------------------------------------------------------------------------------ dW
class DwRun:
    """Device buffers of one weight-gradient problem: dy [B, n_out], x [B, n_in], one position."""

    def __init__(self, n_out, n_in, dy, x, w_off, b_off, size, wide):
        self.n_out, self.n_in, self.size = n_out, n_in, size
        self.lddy, self.ldx = n_out + (5 if wide else 0), n_in + (3 if wide else 0)
        self.DY, self.X = Mat(len(dy), n_out, self.lddy, dy), Mat(len(x), n_in, self.ldx, x)
        self.wo, self.bo = dev(w_off), dev(b_off)

    def run(self, cond, padded=False, fill=None, null_reductions=False):
        """-> bits of the gradient arena [size] after one call over sentinel-filled gradients; scratch filled with `fill`"""
        t = CC.tables(cond, padded)
        tot = self.n_in * self.n_out + self.n_out
        slots = int((-2 - t["chunk_dst"]).max()) + 1 if (t["chunk_dst"] <= -2).any() else 0
        grads, part = Vec(self.size), Vec(max(slots, 1) * tot)
        if fill is not None:
            part.set(np.full(part.cols, fill))
        d = {k: dev(v) for k, v in t.items() if k != "present"}
        red = {} if null_reductions else dict(n_red=len(t["red_cond"]), red_cond=d["red_cond"], red_slot=d["red_slot"],
                                              red_n=d["red_n"], partials=part)
        assert call(DW, n_chunks=len(t["chunk_dst"]), chunk_dst=d["chunk_dst"], chunk_beg=d["chunk_beg"],
                    chunk_end=d["chunk_end"], rows=d["rows"], n_in=self.n_in, n_out=self.n_out, dy=self.DY, lddy=self.lddy,
                    x=self.X, ldx=self.ldx, grads=grads, w_off=self.wo, b_off=self.bo, **red) == 0
        assert grads.slack_untouched() and part.slack_untouched()
        if null_reductions:
            assert part.untouched()
        else:
            assert (part.bits()[0, slots * tot:] == (SENT if fill is None else np.float32(fill).view(np.uint32))).all()
        return grads.bits()[0]


def arena_held(entry, case, bits, G, n, S):
    """present blocks: values inside the bound; everything else: the sentinel"""
    absent = np.isnan(G)
    assert absent.any() and (bits[absent] == SENT).all(), "absent blocks and gaps must not be written"
    held(entry, case, bits.view(np.float32), G, n, S)


@pytest.mark.parametrize("case", CC.DW_CASES, ids=lambda c: f"{c.n_out}x{c.n_in}-{c.B}-{c.layout}-{c.data}")
def test_dw_and_db_of_the_present_blocks(case):
    print(f"\n{case}")
    inp = CC.dw_inputs(case)
    G, S, n = R.weight_grad(inp["dy"], inp["x"], inp["cond"], inp["w_off"], inp["b_off"], inp["size"])
    run = DwRun(case.n_out, case.n_in, inp["dy"], inp["x"], inp["w_off"], inp["b_off"], inp["size"], case.wide)
    # n_red = 0 with NULL reduction arrays and no scratch where no block has more than one piece
    null = not case.padded and not len(CC.tables(inp["cond"])["red_cond"])
    bits = run.run(inp["cond"], case.padded, null_reductions=null)
    arena_held("bwd_dw", case, bits, G, n, S)
    # bitwise reproducible, whatever the scratch slots held; the other table form gives the same bits
    assert np.array_equal(run.run(inp["cond"], case.padded, fill=-3.0e38), bits)
    assert np.array_equal(run.run(inp["cond"], not case.padded, fill=7.0), bits)


@pytest.mark.parametrize("n_out,n_in", [(7, 9), (70, 130)])
def test_dw_of_a_block_does_not_depend_on_the_cells_of_other_blocks(n_out, n_in):
    """The cells of block c keep their batch order; all others are shuffled between them and given other labels: dW[c] and
    db[c] keep their bits (a chain in cell order inside each chunk, the chunk partials added in piece order)."""
    case = next(c for c in CC.DW_CASES if (c.n_out, c.n_in, c.layout, c.data) == (n_out, n_in, "runs", "random"))
    inp = CC.dw_inputs(case)
    cond, B = inp["cond"], case.B
    first = DwRun(n_out, n_in, inp["dy"], inp["x"], inp["w_off"], inp["b_off"], inp["size"], False).run(cond)
    rng = np.random.default_rng(5)
    counts = np.bincount(cond)
    for cells in (1, 33, 65, 257):                   # one chunk; 2, 3 and 9 pieces
        c = int(np.flatnonzero(counts == cells)[0])
        mine, others = np.flatnonzero(cond == c), rng.permutation(np.flatnonzero(cond != c))
        places = np.zeros(B, bool)
        places[rng.choice(B, cells, replace=False)] = True
        order = np.empty(B, np.int64)
        order[places], order[~places] = mine, others
        moved = np.where(places, c, rng.choice(np.delete(np.arange(len(inp["w_off"])), c), B)).astype(np.int32)
        assert not np.array_equal(order, np.arange(B)) and (moved[~places] != cond[order][~places]).any()
        bits = DwRun(n_out, n_in, inp["dy"][order], inp["x"][order], inp["w_off"], inp["b_off"], inp["size"], False).run(moved)
        for off, size in ((inp["w_off"][c], n_out * n_in), (inp["b_off"][c], n_out)):
            assert np.array_equal(bits[off:off + size], first[off:off + size]), cells
            assert (first[off:off + size] != SENT).all()


@pytest.mark.parametrize("case", CC.MULTI_DW, ids=lambda c: f"{c.form}-{c.data}")
def test_dw_multi_in_the_two_layouts_of_the_engine(case):
    """mmvae_cond_linear_bwd_dw_multi as engine_cond.emit_backward calls it.  "deferred" (sequential order): dy [n - 1, R, Z]
    with lddy = Z and dy_pos_stride = R Z, x [n, R, Z] with x_pos_stride = R Z, tables from position 1 on, the scratch
    advanced by one position; position 0 by a single-position call.  "parallel": one x for all (x_pos_stride = 0), dy the
    column blocks of one wide matrix.  Both: the bits of one mmvae_cond_linear_bwd_dw per position."""
    print(f"\n{case}")
    inp = CC.multi_dw_inputs(case)
    n, R_, Z, cond = case.n_pos, case.R, case.Z, inp["cond"]
    G, S, cnt = R.weight_grad(inp["dy"], inp["x"], cond, inp["w_off"], inp["b_off"], inp["size"])
    wo, bo = dev(inp["w_off"]), dev(inp["b_off"])
    P, lay = CT.words(R_), CT.layout(R_)
    pack = np.zeros(n * P, np.int32)
    for j in range(n):
        CT.fill_padded(pack[j * P:(j + 1) * P], CT.group_tables(cond[j]), R_)
    tbl = dev(pack)
    at = lambda j, name: tbl.data_ptr() + 4 * (j * P + lay[name])  # noqa: E731
    tables = lambda j: {k: at(j, k) for k in ("chunk_dst", "chunk_beg", "chunk_end", "rows", "red_cond", "red_slot", "red_n")}  # noqa: E731
    n_chunks, n_red = CT.max_chunks(R_), CT.max_reductions(R_)
    part_stride = CT.partial_slots(R_) * (Z * Z + Z)
    if case.form == "deferred":
        X, DY = Mat(n * R_, Z, Z, inp["x"]), Mat(n * R_, Z, Z, inp["dy"])
        lddy, dps, xps = Z, R_ * Z, R_ * Z
        x_at = lambda j: X.ptr() + 4 * j * R_ * Z    # noqa: E731
        dy_at = lambda j: DY.ptr() + 4 * j * R_ * Z  # noqa: E731
    else:
        wide = blocks_in_columns(inp["dy"], Z)
        X, DY = Mat(R_, Z, Z + 3, inp["x"]), Mat(R_, n * Z, n * Z + 5, wide)
        lddy, dps, xps = n * Z + 5, Z, 0
        x_at = lambda j: X.ptr()                     # noqa: E731
        dy_at = lambda j: DY.ptr() + 4 * j * Z       # noqa: E731
    ldx = X.ld

    def one(j, grads, part, at_part):
        assert call(DW, n_chunks=n_chunks, n_in=Z, n_out=Z, dy=dy_at(j), lddy=lddy, x=x_at(j), ldx=ldx, grads=grads, w_off=wo,
                    b_off=bo, n_red=n_red, partials=at_part, **tables(j)) == 0
        assert grads.slack_untouched() and part.slack_untouched()

    singles, part = Vec(inp["size"]), Vec(part_stride)
    for j in range(n - 1, -1, -1):
        one(j, singles, part, part)
    arena_held("bwd_dw, per position", case, singles.bits()[0], G, cnt, S)
    grads, part = Vec(inp["size"]), Vec(n * part_stride)
    first = 1 if case.form == "deferred" else 0
    assert call("mmvae_cond_linear_bwd_dw_multi", n_pos=n - first, n_chunks=n_chunks, tbl_stride=P, n_in=Z, n_out=Z,
                dy=dy_at(first), lddy=lddy, dy_pos_stride=dps, x=x_at(first), ldx=ldx, x_pos_stride=xps, grads=grads, w_off=wo,
                b_off=bo, n_red=n_red, partials=part.ptr() + 4 * first * part_stride, part_pos_stride=part_stride,
                **tables(first)) == 0
    if first:
        # nothing of position 0 yet: its blocks and its scratch still hold the sentinel
        G0 = R.weight_grad(inp["dy"][:1], inp["x"][:1] if inp["x"].ndim == 3 else inp["x"], cond[:1], inp["w_off"],
                           inp["b_off"], inp["size"])[0]
        assert (grads.bits()[0][~np.isnan(G0)] == SENT).all() and (part.bits()[0, :part_stride] == SENT).all()
        one(0, grads, part, part)
    assert grads.slack_untouched() and part.slack_untouched()
    arena_held("bwd_dw_multi", case, grads.bits()[0], G, cnt, S)
    assert np.array_equal(grads.bits(), singles.bits())


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_six_entries_leaves_the_outputs_alone():
    """Each MMVAE_ERR_ARG condition written in the six entries, one call each, over outputs that hold sentinels before and
    after.  The unbroken argument lists are accepted (on other outputs) first.  Every refusal precedes the first launch,
    so the sizes named here are never touched."""
    from mmvae_amd import _lib

    B, Z, n = 40, 16, 2                              # one block of 40 cells: two chunks, one reduction
    rng = np.random.default_rng(2)
    w_off, b_off, size = CC.offsets_only(rng, 2, Z, Z)
    params = dev(CC.values(rng, "random", size))
    wo, bo = dev(w_off), dev(b_off)
    v = Mat(B, n * Z, n * Z, CC.values(rng, "random", (B, n * Z)))  # x, dy: wide enough for two positions
    tabs = [CC.tables(np.full(B, j, np.int32)) for j in range(n)]  # position j: every cell in block j
    tbl, at = table_pack([{k: a for k, a in t.items() if k != "present"} for t in tabs], 6 * B)
    tot = Z * Z + Z

    def outputs():
        return dict(y=Mat(B, n * Z, n * Z), dx=Mat(B, Z, Z), grads=Vec(size), part=Vec(n * 2 * tot))

    def lists(o):
        dw = dict(n_chunks=2, chunk_dst=at["chunk_dst"], chunk_beg=at["chunk_beg"], chunk_end=at["chunk_end"],
                  rows=at["rows"], n_in=Z, n_out=Z, dy=v, lddy=n * Z, x=v, ldx=n * Z, grads=o["grads"], w_off=wo, b_off=bo,
                  n_red=1, red_cond=at["red_cond"], red_slot=at["red_slot"], red_n=at["red_n"], partials=o["part"])
        return {
            FWD: dict(B=B, n_in=Z, n_out=Z, x=v, ldx=n * Z, params=params, w_off=wo, b_off=bo, cond=at["cond"],
                      rows=at["rows"], y=o["y"], ldy=n * Z),
            DX: dict(B=B, n_in=Z, n_out=Z, dy=v, lddy=n * Z, params=params, w_off=wo, cond=at["cond"], rows=at["rows"],
                     dx=o["dx"], lddx=Z),
            DW: dw,
            "mmvae_cond_linear_fwd_multi": dict(n_pos=n, B=B, n_in=Z, n_out=Z, x=v, ldx=n * Z, params=params, w_off=wo,
                                                b_off=bo, cond=at["cond"], rows=at["rows"], tbl_stride=6 * B, y=o["y"],
                                                ldy=n * Z, y_pos_stride=Z),
            "mmvae_cond_linear_bwd_dx_multi": dict(n_pos=n, B=B, n_in=Z, n_out=Z, dy=v, lddy=n * Z, dy_pos_stride=Z,
                                                   params=params, w_off=wo, cond=at["cond"], tbl_stride=6 * B, dx=o["dx"],
                                                   lddx=Z),
            "mmvae_cond_linear_bwd_dw_multi": dict(dw, n_pos=n, tbl_stride=6 * B, dy_pos_stride=Z, part_pos_stride=2 * tot),
        }

    for name, kw in lists(outputs()).items():
        assert call(name, **kw) == 0, name
    o = outputs()
    base = lists(o)
    shape = [dict(B=0), dict(n_in=0), dict(n_out=0)]
    positions = [dict(n_pos=0), dict(n_pos=65)]
    dw = [dict(n_chunks=0), dict(n_in=0), dict(n_out=0), dict(chunk_dst=None), dict(chunk_beg=None), dict(chunk_end=None),
          dict(rows=None), dict(dy=None), dict(x=None), dict(grads=None), dict(w_off=None), dict(b_off=None),
          dict(lddy=Z - 1), dict(ldx=Z - 1), dict(n_red=-1), dict(red_cond=None), dict(red_slot=None), dict(red_n=None),
          dict(partials=None),
          dict(n_in=32768, n_out=32768, lddy=32768, ldx=32768),                # 65536 tiles
          dict(n_in=128 * 65535, n_out=128, lddy=128, ldx=128 * 65535)]        # 65535 tiles, too many reduction groups
    refusals = {
        FWD: shape + [dict(n_in=8193, ldx=8193), dict(x=None), dict(params=None), dict(w_off=None), dict(b_off=None),
                      dict(cond=None), dict(y=None), dict(ldx=Z - 1), dict(ldy=Z - 1)],
        DX: shape + [dict(n_out=8193, lddy=8193), dict(dy=None), dict(params=None), dict(w_off=None), dict(cond=None),
                     dict(dx=None), dict(lddy=Z - 1), dict(lddx=Z - 1)],
        DW: dw,
        "mmvae_cond_linear_fwd_multi": shape + positions + [
            dict(n_in=257, ldx=257), dict(x=None), dict(params=None), dict(w_off=None), dict(b_off=None), dict(cond=None),
            dict(rows=None), dict(y=None), dict(ldx=Z - 1), dict(ldy=Z - 1), dict(tbl_stride=B - 1)],
        "mmvae_cond_linear_bwd_dx_multi": shape + positions + [
            dict(n_out=1025, lddy=1025 + Z), dict(dy=None), dict(params=None), dict(w_off=None), dict(cond=None),
            dict(dx=None), dict(lddy=2 * Z - 1), dict(lddx=Z - 1), dict(tbl_stride=B - 1),
            dict(n_pos=64, n_out=256, dy_pos_stride=256, lddy=64 * 256)],       # 64 x 256 + 128 floats of LDS > 64 KB
        "mmvae_cond_linear_bwd_dw_multi": positions + dw,
    }
    for name, cases in refusals.items():
        for over in cases:
            assert call(name, **dict(base[name], **over)) == _lib.ERR_ARG, (name, over)
    assert all(buf.untouched() for buf in o.values()), [k for k, buf in o.items() if not buf.untouched()]
