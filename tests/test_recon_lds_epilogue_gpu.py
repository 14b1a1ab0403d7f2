"""The reconstruction epilogue of the wave-specialised kernel (csrc/gemm_dev.h, recon_lds_epilogue): the accumulators
leave the registers as four 64-row slices through one LDS image and all 512 threads -- multipliers and stagers -- turn a
slice into xhat, dP, the dP planes and the two partial sums.

Inputs are integer-valued (|h|, |W| <= 3, 0 <= x < 256, |bias| <= 8, H <= 96): every bf16 piece, product and sum of
P = h W^T + bias is exact in fp32, so xhat and dP must EQUAL the fp64 reference -- a wrong row, column, slice or x row
shows up as a different integer, not as rounding.  The partial sums are rounded fp32 sums (se_part: up to 160 squares of
up to ~1100^2 per entry) and are held to the bounds of tests/test_kernels_gpu.py::test_decoder_recon (gemm_state_cases);
the kernel adds them in the order of the register epilogue it replaced (bitwise the same se_part and col_part).

Shapes are the smallest that reach the kernel (>= 160 work items) with two row tiles, the second 4 rows high, and a
ragged last column tile.  Before a case launches it asks the planner for the tile count of the tile it names, and after
the launch the zero rows of se_part must be those of that tile's width: a case cannot silently run another kernel."""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_state_cases as S  # noqa: E402
from tests.gemm_state_cases import COL_PART_REL, NT, SE_DP_REL, W256x128, W256x160, gemm_state  # noqa: E402

R = 260          # two 256-row tiles, the second with 4 valid rows (and rows 256..259 = a third 128-row half)
G160 = 16404     # 103 column tiles of 160, the last 84 wide: 206 items; 2 * ceil(G / 128) = 258 > 256 slots
G128 = 10244     # 81 column tiles of 128, the last 4 wide: 162 items


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from mmvae_amd import ops as _ops, _lib

    _lib.load()
    yield _ops
    data.cache_clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def state_is_restored():
    yield
    S.assert_default_state()


def ints(*shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def data(B, G, H, with_bias=True):
    """inputs on the device and the fp64 reference (computed once, on the CPU) of the R-row launch over B rows of x"""
    h, W = ints(R, H, lo=-3, hi=3, seed=1), ints(G, H, lo=-3, hi=3, seed=2)
    bias = ints(G, lo=-8, hi=8, seed=3) if with_bias else None
    x = ints(B, G, lo=0, hi=255, seed=4)
    P = h.double() @ W.double().t()
    if with_bias:
        P = P + bias.double()
    assert float(P.abs().max()) + 255 < 2 ** 11  # (exact in fp32 by a wide margin)
    d = types.SimpleNamespace(h=h.cuda(), W=W.cuda(), bias=bias.cuda() if with_bias else None, x=x.cuda())
    xh = P.clamp_min(0)
    diff = xh - x.double().repeat(R // B, 1)
    d.xhat = xh.float().cuda()
    d.dP = (2 * diff * (P > 0)).float().cuda()
    assert 0.2 < float((P > 0).double().mean()) < 0.8  # both sides of the ReLU
    d.se = (diff * diff).sum(1).cuda()                                       # [R], fp64
    d.col = torch.stack([d.dP[128 * t:128 * (t + 1)].double().sum(0) for t in range(S.ceil_div(R, 128))])  # [3, G]
    return d


def rel(a, b):
    b = b.double()
    return float((a.double() - b).norm() / b.norm())


def planned(lib, G, H, tile):
    assert lib.mmvae_gemm_sq_partials(NT, R, G, H, 0) == S.tiles(R, G, tile), "the case does not reach the tile it names"


def check(ops, d, G, tile, xhat, dP, se_part, col_part=None):
    """the outputs of one launch against the reference; `tile`: the tile the launch must have run"""
    nt = S.ceil_div(G, tile[1])
    assert se_part.shape == (ops.recon_tiles(G), R)
    assert bool((se_part[:nt] > 0).all()) and bool((se_part[nt:] == 0).all()), "se_part rows of another tiling"
    assert rel(se_part.double().sum(0), d.se) <= SE_DP_REL
    if xhat is not None:
        assert torch.equal(xhat, d.xhat)
    if dP is not None:
        assert torch.equal(dP, d.dP)
    if col_part is not None:
        for t in range(col_part.shape[0]):
            assert rel(col_part[t], d.col[t]) <= COL_PART_REL, t


def launch(ops, d, **kw):
    """(xhat, dP, se_part, col_part) of one launch; se_part and col_part start as NaN: every entry is the call's"""
    G = d.W.shape[0]
    se = torch.full((ops.recon_tiles(G), R), float("nan"), device="cuda")
    col = torch.full((ops.recon_row_tiles(R), G), float("nan"), device="cuda") if kw.pop("want_col", True) else None
    xhat, dP, se = ops.decoder_recon(d.h, d.W, d.bias, d.x, se_part=se, col_part=col, **kw)
    return xhat, dP, se, col


# 1 - 4: one round, one item per workgroup.  H = 64 / 96: two / three k-tiles, so the image the epilogue takes over is
# image 1 / image 0.
@pytest.mark.parametrize("B,G,H,tile", [
    (R, G160, 64, W256x160),      # 1. 256x160: two row tiles, ragged last column tile
    (R, G160 - 2, 96, W256x160),  # 2. G % 4 != 0: the 4-gene group that straddles the edge
    (R // 2, G160, 64, W256x160), # 3. K-sample rows: x is read modulo 130 rows
    (R, G128, 96, W256x128),      # 4. the 2 x 2 instantiation: two slices per multiplier wave
])
def test_one_round(ops, B, G, H, tile):
    d = data(B, G, H)
    with gemm_state(x3w=1) as lib:
        planned(lib, G, H, tile)
        out = launch(ops, d)
    check(ops, d, G, tile, *out)


# 5. several items per workgroup: the stagers have the next item's first k-tile in the other image while the epilogue runs
def test_capped_to_40_workgroups(ops):
    """40 workgroups: the planner moves case 1 to 256x128 (258 items, 7 rounds x 32768 against 6 x 40960) -- held to
    fp64 -- and keeps case 4 on it, whose outputs must be bitwise those of the uncapped launch of the same tile"""
    d = data(R, G160, 64)
    with gemm_state(x3w=1, cap=40) as lib:
        planned(lib, G160, 64, W256x128)
        out = launch(ops, d)
    check(ops, d, G160, W256x128, *out)
    d = data(R, G128, 96)
    with gemm_state(x3w=1) as lib:
        planned(lib, G128, 96, W256x128)
        want = launch(ops, d)
    with gemm_state(x3w=1, cap=40) as lib:
        planned(lib, G128, 96, W256x128)
        got = launch(ops, d)
    check(ops, d, G128, W256x128, *got)
    for name, a, b in zip(("xhat", "dP", "se_part", "col_part"), got, want):
        assert torch.equal(a, b), name


def test_capped_256x160_is_bitwise_the_uncapped_launch(ops):
    """103 workgroups x two items of case 1 (2 rounds x 40960 against 3 x 32768 for 258 of 256x128): the same tile, so
    the same partial sums bit for bit whichever workgroup and round runs an item"""
    d = data(R, G160, 64)
    with gemm_state(x3w=1) as lib:
        planned(lib, G160, 64, W256x160)
        want = launch(ops, d)
    with gemm_state(x3w=1, cap=103) as lib:
        planned(lib, G160, 64, W256x160)
        got = launch(ops, d)
    check(ops, d, G160, W256x160, *got)
    for name, a, b in zip(("xhat", "dP", "se_part", "col_part"), got, want):
        assert torch.equal(a, b), name


# 6. output subsets of case 1
def test_output_subsets(ops):
    d = data(R, G160, 64)
    with gemm_state(x3w=1) as lib:
        planned(lib, G160, 64, W256x160)
        full = launch(ops, d)
        no_xhat = launch(ops, d, want_xhat=False)
        no_col = launch(ops, d, want_col=False)
        nothing = launch(ops, d, want_xhat=False, want_dP=False, want_col=False)
    check(ops, d, G160, W256x160, *full)
    assert no_xhat[0] is None and no_col[3] is None and nothing[0] is None and nothing[1] is None
    for out in (no_xhat, no_col, nothing):
        check(ops, d, G160, W256x160, *out)
        assert torch.equal(out[2], full[2])  # the squared errors do not depend on what else is stored


def test_dp_as_planes_only(ops):
    """dP = null, dP planes out (G % 8 == 0): the three bf16 planes add up to the reference dP exactly"""
    G = G160 - 4
    d = data(R, G, 64)
    with gemm_state(x3w=1) as lib:
        planned(lib, G, 64, W256x160)
        planes = ops.Planes(R, G, "cuda")
        xhat, dP, se, col = launch(ops, d, want_dP=False, dP_planes=planes)
        both = ops.Planes(R, G, "cuda")
        out = launch(ops, d, dP_planes=both)
    assert dP is None
    check(ops, d, G, W256x160, xhat, dP, se, col)
    assert torch.equal(planes.to_float(), d.dP)
    check(ops, d, G, W256x160, *out)
    assert torch.equal(both.data, planes.data)


def test_without_bias(ops):
    d = data(R, G160, 64, with_bias=False)
    with gemm_state(x3w=1) as lib:
        planned(lib, G160, 64, W256x160)
        out = launch(ops, d)
    check(ops, d, G160, W256x160, *out)


# 7. the planes-operand launches (launch_x3w_planes): h pre-split, then W too -- the stagers only move planes
@pytest.mark.parametrize("G,H,tile", [(G160, 64, W256x160), (G128, 96, W256x128)])
def test_planes_operands(ops, G, H, tile):
    d = data(R, G, H)
    hp, wp = ops.split_planes(d.h), ops.split_planes(d.W)
    with gemm_state(x3w=1) as lib:
        planned(lib, G, H, tile)
        want = launch(ops, d)
        got_h = launch(ops, d, h_planes=hp)
        got_hw = launch(ops, d, h_planes=hp, W_planes=wp)
    for got in (got_h, got_hw):
        check(ops, d, G, tile, *got)
        for name, a, b in zip(("xhat", "dP", "se_part", "col_part"), got, want):
            assert torch.equal(a, b), name
