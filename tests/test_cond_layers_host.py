"""The restatement of the conditional-layer kernels (tests/cond_restatement.py) and the cases of
tests/test_cond_layers_gpu.py (tests/cond_cases.py), checked without a GPU.

1. In float64 the restatement equals a per-condition torch loop with autograd -- for every condition present in the batch:
   index_select, Linear, index_copy_, which is what the reference's ConditionalLayer.forward does -- within 1e-12 of the
   largest reference value, and leaves exactly the absent blocks and the gaps of the gradient arena without a value.
2. The case lists reach the classes of csrc/cond_layers.hip that the GPU file's docstring names: plain assertions over the
   tuples, their tables (cond_tables.group_tables) and their arenas.
3. The bound of the GPU file, |device - fp64| <= (n + 3) 2^-24 S per element, is not vacuous: the restatement evaluated in
   float32 in the kernels' documented order stays inside it on every random case (the largest ratio is printed), and on the
   exact data the float32 evaluation equals the float64 one bit for bit.
"""
import numpy as np
import pytest
import torch

from mmvae_amd import cond_tables as CT
from tests import cond_cases as CC
from tests import cond_restatement as R

REL = 1e-12


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)
    assert err <= REL, err


def torch_loop(x, arena, w_off, b_off, cond, n_out, dy):
    """One Linear per block, applied condition by condition.  x [n_pos, B, n_in] (or one [B, n_in] for all positions),
    cond [n_pos, B] -> y [n_pos, B, n_out], the gradient of sum(y dy) with respect to x, {block: (dW, db)}."""
    cond = np.atleast_2d(cond)
    x = torch.from_numpy(np.array(x)).double().requires_grad_(True)
    n_in = x.shape[-1]
    layers = {}
    for c in np.unique(cond):
        lin = torch.nn.Linear(n_in, n_out).double()
        lin.weight.data.copy_(torch.from_numpy(np.array(R.block(arena, w_off, c, n_out, n_in))))
        lin.bias.data.copy_(torch.from_numpy(np.array(R.block(arena, b_off, c, n_out))))
        layers[int(c)] = lin
    ys = []
    for j in range(cond.shape[0]):
        xj = x if x.dim() == 2 else x[j]
        y = torch.empty(xj.shape[0], n_out, dtype=torch.float64)
        for c in np.unique(cond[j]):
            idx = torch.from_numpy(np.flatnonzero(cond[j] == c))
            y = y.index_copy(0, idx, layers[int(c)](xj.index_select(0, idx)))
        ys.append(y)
    y = torch.stack(ys)
    (y * torch.from_numpy(np.array(dy)).double()).sum().backward()
    grads = {c: (lin.weight.grad.numpy(), lin.bias.grad.numpy()) for c, lin in layers.items()}
    return y.detach().numpy(), x.grad.numpy(), grads


HANDFUL_FWD = [c for c in CC.FWD_CASES if c.data == "random" and (c.n_in, c.n_out) in ((63, 5), (65, 17), (193, 9), (257, 3))]
HANDFUL_DX = [c for c in CC.DX_CASES if c.data == "random" and c.n_out in (1, 7, 17, 129, 1025)]
HANDFUL_DW = [c for c in CC.DW_CASES if c.data == "random" and (c.n_out, c.n_in) in ((1, 1), (8, 200), (129, 127), (7, 9))]


@pytest.mark.parametrize("case", HANDFUL_FWD, ids=lambda c: f"{c.n_in}x{c.n_out}-{c.B}")
def test_forward_restatement_equals_the_torch_loop(case):
    inp = CC.fwd_inputs(case)
    dy = np.ones(inp["cond"].shape + (case.n_out,))
    want, _, _ = torch_loop(inp["x"], inp["arena"], inp["w_off"], inp["b_off"], inp["cond"], case.n_out, dy)
    y, S = R.forward(inp["x"], inp["arena"], inp["w_off"], inp["b_off"], inp["cond"], case.n_out)
    close(y, want)
    assert (S >= np.abs(y)).all() and np.isfinite(S).all()
    # one position of its own is the first of several
    y0, S0 = R.forward(inp["x"][0], inp["arena"], inp["w_off"], inp["b_off"], inp["cond"][0], case.n_out)
    assert np.array_equal(y0[0], y[0]) and np.array_equal(S0[0], S[0])


@pytest.mark.parametrize("case", HANDFUL_DX, ids=lambda c: f"{c.n_in}x{c.n_out}-{c.B}-p{c.n_pos}")
def test_input_gradient_restatement_equals_torch_autograd(case):
    inp = CC.dx_inputs(case)
    b_off = inp["w_off"]  # (any readable floats: the bias does not enter dx)
    x = np.zeros((case.B, case.n_in))
    _, want, _ = torch_loop(x, inp["arena"], inp["w_off"], b_off, inp["cond"], case.n_out, inp["dy"])
    dx, S = R.input_grad(inp["dy"], inp["arena"], inp["w_off"], inp["cond"], case.n_in)
    close(dx, want)
    acc, S_acc = R.input_grad(inp["dy"], inp["arena"], inp["w_off"], inp["cond"], case.n_in, old=inp["old"])
    close(acc, want + inp["old"])
    assert np.array_equal(S_acc, S + np.abs(inp["old"])) and (S_acc >= np.abs(acc) * (1 - 1e-12)).all()


def check_weight_grad(dy, x, cond, w_off, b_off, size, n_out, n_in):
    arena = np.zeros(size, np.float32)  # the values of the parameters do not enter dW
    _, _, grads = torch_loop(x, arena, w_off, b_off, cond, n_out, dy)
    G, S, n = R.weight_grad(dy, x, cond, w_off, b_off, size)
    touched = np.zeros(size, bool)
    for c, (dW, db) in grads.items():
        close(R.block(G, w_off, c, n_out, n_in), dW)
        close(R.block(G, b_off, c, n_out), db)
        cells = int((np.atleast_2d(cond) == c).sum())
        assert (R.block(n, w_off, c, n_out, n_in) == cells).all() and (R.block(n, b_off, c, n_out) == cells).all()
        R.block(touched, w_off, c, n_out, n_in)[:] = True
        R.block(touched, b_off, c, n_out)[:] = True
    assert np.array_equal(np.isnan(G), ~touched) and np.array_equal(np.isnan(S), ~touched) and not n[~touched].any()
    assert len(grads) < len(w_off), "some blocks are absent"


@pytest.mark.parametrize("case", HANDFUL_DW, ids=lambda c: f"{c.n_out}x{c.n_in}-{c.B}")
def test_weight_gradient_restatement_equals_torch_autograd(case):
    inp = CC.dw_inputs(case)
    check_weight_grad(inp["dy"], inp["x"], inp["cond"], inp["w_off"], inp["b_off"], inp["size"], case.n_out, case.n_in)


@pytest.mark.parametrize("case", [c for c in CC.MULTI_DW if c.data == "random"], ids=lambda c: c.form)
def test_weight_gradient_of_several_positions_equals_torch_autograd(case):
    inp = CC.multi_dw_inputs(case)
    check_weight_grad(inp["dy"], inp["x"], inp["cond"], inp["w_off"], inp["b_off"], inp["size"], case.Z, case.Z)


# ------------------------------------------------------------------------------------------------------------ coverage
def both_data(cases, key):
    """the values of `key` over the cases, which must be the same for both kinds of data"""
    sets = [{key(c) for c in cases if c.data == data} for data in CC.DATA]
    assert sets[0] == sets[1]
    return sets[0]


def test_forward_cases_reach_every_class_of_the_sorted_and_the_one_cell_kernel():
    shapes = both_data(CC.FWD_CASES, lambda c: (c.n_in, c.n_out))
    assert shapes == {(1, 1), (63, 5), (64, 4), (65, 17), (128, 128), (129, 3), (192, 16), (193, 9), (256, 31), (257, 3),
                      (8192, 3)}
    n_ins = {s[0] for s in shapes}
    assert {(n + 63) // 64 for n in n_ins if n <= 256} == {1, 2, 3, 4}          # every instantiated T
    assert {64, 65, 128, 129, 192, 193, 256, 257, 8192} <= n_ins                # both sides of every switch, the maximum
    assert {s[1] % 16 for s in shapes} >= {0, 1, 3, 4, 5, 9, 15}                # ragged and full slices of FW_RO = 16 rows
    assert {s[1] > 16 for s in shapes} == {True, False}                         # one and several slices
    assert both_data(CC.FWD_CASES, lambda c: c.B) == set(CC.B_VALUES)
    assert both_data(CC.FWD_CASES, lambda c: c.layout) == set(CC.LAYOUTS)
    assert both_data(CC.FWD_CASES, lambda c: c.wide) == {True, False}
    shared = differing = False
    for c in CC.FWD_CASES:
        inp = CC.fwd_inputs(c)
        assert inp["cond"].shape == ((CC.FWD_N_POS if c.n_in <= 256 else 1), c.B)  # n_pos 1 and 3 of _fwd_multi
        assert len(np.unique(inp["cond"])) < len(inp["w_off"])                     # absent blocks
        assert {int(o) % 4 for o in inp["w_off"]} == {0, 1, 2, 3}
        first = inp["cond"][0][CT.group_tables(inp["cond"][0])["rows"][:8]]        # the first set of FW_CB sorted cells
        shared |= len(first) == 8 and len(set(first)) == 1
        differing |= len(first) == 8 and len(set(first)) == 8
    assert shared and differing


def test_dx_cases_reach_every_class_of_the_three_kernels():
    n_outs = both_data(CC.DX_CASES, lambda c: c.n_out)
    assert n_outs == {1, 7, 15, 16, 17, 129, 1024, 1025, 8192}
    assert {c.n_in for c in CC.DX_CASES if c.n_out >= 1024} == {5, 3}
    n_ins = both_data(CC.DX_CASES, lambda c: c.n_in)
    assert {1, 127, 128, 129, 257} <= n_ins and {(n + 127) // 128 for n in n_ins} == {1, 2, 3}  # passes of DX_K
    halves = {((n + 1) // 2, n // 2) for n in n_outs}                           # rows of the lower and the upper half
    assert (1, 0) in halves                                                     # an empty upper half
    assert any(lo != hi for lo, hi in halves) and any(lo == hi for lo, hi in halves)      # odd and even n_out
    assert any(0 < hi < 8 for lo, hi in halves) and any(lo < 8 for lo, hi in halves)      # a half below one DX_U batch
    assert any(h >= 8 and h % 8 for pair in halves for h in pair)               # batches and a remainder in one half
    assert any(h >= 8 and h % 8 == 0 for pair in halves for h in pair)          # batches alone
    assert {1024, 1025} <= n_outs                                               # the switch of _bwd_dx, the maximum 8192
    assert both_data([c for c in CC.DX_CASES if c.n_out <= 1024], lambda c: c.n_pos) == {1, 2, 6}
    assert {c.n_pos for c in CC.DX_CASES if c.n_out > 1024} == {1}              # (_bwd_dx_multi refuses those)
    assert both_data(CC.DX_CASES, lambda c: c.B) == set(CC.B_VALUES)
    assert both_data(CC.DX_CASES, lambda c: c.layout) == set(CC.LAYOUTS)
    assert both_data(CC.DX_CASES, lambda c: c.wide) == {True, False}
    uniform = split = ragged = False
    for c in CC.DX_CASES:
        cond = CC.dx_inputs(c)["cond"][0]
        sets = [cond[CT.group_tables(cond)["rows"][i:i + 8]] for i in range(0, c.B, 8)]   # the sets of DX_CB sorted cells
        uniform |= any(len(s) == 8 and len(set(s)) == 1 for s in sets)
        split |= any(len(s) == 8 and len(set(s)) > 1 for s in sets)
        ragged |= any(len(s) < 8 for s in sets)
    assert uniform and split and ragged


def test_dw_cases_reach_every_tile_chunk_piece_and_offset_class():
    shapes = both_data(CC.DW_CASES, lambda c: (c.n_out, c.n_in))
    assert shapes == {(1, 1), (8, 200), (128, 128), (129, 127), (130, 260), (70, 130), (7, 9)}
    assert {((o + 127) // 128, (k + 127) // 128) for o, k in shapes} >= {(1, 1), (2, 1), (2, 3), (1, 2)}
    assert {k % 4 for _, k in shapes} == {0, 1, 2, 3}
    assert both_data(CC.DW_CASES, lambda c: c.B) == set(CC.B_VALUES)
    assert both_data(CC.DW_CASES, lambda c: c.layout) == set(CC.LAYOUTS)
    assert both_data(CC.DW_CASES, lambda c: c.padded) == {True, False}
    assert both_data(CC.DW_CASES, lambda c: c.wide) == {True, False}
    assert sum(CC.RUN_COUNTS) == 901
    aligned_rows, no_reduction = set(), set()
    for c in CC.DW_CASES:
        inp = CC.dw_inputs(c)
        t = CC.tables(inp["cond"])
        counts = np.bincount(inp["cond"])[t["present"]]
        assert len(t["present"]) < len(inp["w_off"])                                # absent blocks
        sizes = t["chunk_end"] - t["chunk_beg"]
        assert sizes.min() >= 1 and sizes.max() <= CT.CHUNK and sizes.sum() == c.B
        if c.layout == "runs":
            assert (c.n_out, c.n_in) in ((7, 9), (70, 130))
            assert sorted(counts) == sorted(CC.RUN_COUNTS) and len(sizes) == 34
            assert sorted(t["red_n"]) == [2, 2, 3, 4, 5, 6, 9]                      # 2 .. 6 and 9 pieces
            assert {1, 31, 32} <= set(sizes)                                        # a one-cell, a ragged and a full chunk
            assert not np.array_equal(np.sort(inp["cond"]), inp["cond"])            # shuffled labels
        if c.layout == "distinct":
            assert len(sizes) == c.B and not len(t["red_n"])
        if not len(t["red_n"]) and not c.padded:
            no_reduction.add(c.data)                                                # n_red = 0 with NULL arrays
        if c.padded:
            p = CC.tables(inp["cond"], padded=True)
            assert len(p["chunk_dst"]) == CT.max_chunks(c.B) > len(sizes) and (p["chunk_dst"][len(sizes):] == -1).all()
            assert len(p["red_cond"]) == CT.max_reductions(c.B) > len(t["red_n"])
            assert (p["red_cond"][len(t["red_n"]):] == -1).all()
        for blk in t["present"]:                                                    # weight and bias are not adjacent
            assert inp["w_off"][blk] + c.n_out * c.n_in != inp["b_off"][blk] != inp["w_off"][blk] - c.n_out
        if c.n_in % 4 == 0:  # a weight row keeps the residue of its block: 16-byte stores (0) and element stores (1, 2, 3)
            aligned_rows |= {(c.data, int(inp["w_off"][blk]) % 4) for blk in t["present"]}
    assert no_reduction == set(CC.DATA)
    assert aligned_rows == {(d, r) for d in CC.DATA for r in range(4)}
    for c in CC.MULTI_DW:
        inp = CC.multi_dw_inputs(c)
        pieces = [sorted(CC.tables(cond)["red_n"]) for cond in inp["cond"]]
        assert [3] in pieces and [] in pieces                                       # positions with and without reductions
        assert inp["x"].ndim == (3 if c.form == "deferred" else 2)
    assert {(c.form, c.data) for c in CC.MULTI_DW} == {(f, d) for f in ("deferred", "parallel") for d in CC.DATA}


def test_arena_gaps_cycle_through_every_residue():
    rng = np.random.default_rng(0)
    arena, w_off, b_off = CC.make_arena(rng, "random", 9, 4, 8)
    spans = sorted([(int(o), 32) for o in w_off] + [(int(o), 4) for o in b_off])
    gaps = [spans[0][0]] + [b[0] - (a[0] + a[1]) for a, b in zip(spans, spans[1:])]
    assert [g % 4 for g in gaps[1:]] == [i % 4 for i in range(1, len(spans))] and min(gaps) == 0
    used = np.zeros(arena.size, bool)
    for o, n in spans:
        assert not used[o:o + n].any()
        used[o:o + n] = True
    assert (arena.view(np.uint32)[~used] == CC.SENT).all() and np.isfinite(arena[used]).all() and not used[-3:].any()


# ------------------------------------------------------------------------------------ the bound is not vacuous
def inside(name, case, f32, f64, n, S):
    f64 = np.asarray(f64, np.float64)
    ok = ~np.isnan(f64)
    assert np.array_equal(np.isnan(f32), ~ok)
    if case.data == "exact":
        assert np.array_equal(f32[ok].astype(np.float64), f64[ok]), name
        return
    dev, lim = np.abs(f32[ok].astype(np.float64) - f64[ok]), R.bound(n, S)[ok] if np.ndim(n) else R.bound(n, S[ok])
    assert (dev <= lim).all(), (name, case)
    ratio = float((dev / np.where(lim > 0, lim, 1.0)).max())
    print(f"  {name} {case}: float32 restatement at {ratio:.3f} of the bound")


@pytest.mark.parametrize("case", CC.FWD_CASES, ids=lambda c: f"{c.n_in}x{c.n_out}-{c.B}-{c.data}")
def test_forward_in_float32_stays_inside_the_bound_and_is_exact_on_integers(case):
    inp = CC.fwd_inputs(case)
    args = (inp["x"], inp["arena"], inp["w_off"], inp["b_off"], inp["cond"], case.n_out)
    y, S = R.forward(*args)
    inside("y", case, R.forward_f32(*args), y, case.n_in, S)


@pytest.mark.parametrize("case", CC.DX_CASES, ids=lambda c: f"{c.n_in}x{c.n_out}-{c.B}-p{c.n_pos}-{c.data}")
def test_dx_in_float32_stays_inside_the_bound_and_is_exact_on_integers(case):
    inp = CC.dx_inputs(case)
    for old in (None, inp["old"]):
        args = (inp["dy"], inp["arena"], inp["w_off"], inp["cond"], case.n_in, old)
        dx, S = R.input_grad(*args)
        inside("dx", case, R.input_grad_f32(*args), dx, case.n_pos * case.n_out + (old is not None), S)


@pytest.mark.parametrize("case", CC.DW_CASES + CC.MULTI_DW, ids=str)
def test_dw_in_float32_stays_inside_the_bound_and_is_exact_on_integers(case):
    inp = CC.dw_inputs(case) if isinstance(case, CC.DwCase) else CC.multi_dw_inputs(case)
    args = (inp["dy"], inp["x"], inp["cond"], inp["w_off"], inp["b_off"], inp["size"])
    G, S, n = R.weight_grad(*args)
    inside("dW, db", case, R.weight_grad_f32(*args), G, n, S)
