"""The chip-filling GEMMs and the fused reconstruction kernel in the launch states the other kernel tests never set
(tests/gemm_state_cases.py): the 2 x 4-wave bf16x3 family (x3w = 0: what every data-parallel run launches), the
persistent kernel under a workgroup cap (the single-rank step's side branches) and exact-f32 products.

Every product is held to an fp64 product computed once per shape on the CPU (the comparisons themselves run on the
device, in fp64); bounds are the project's own (gemm_state_cases.py).  Before a case launches it asks the planner, on
the device, for the tile count the host-only test pinned: a case that silently took another kernel fails there.
Calls go through the C-ABI (mmvae_amd.ops -> ctypes -> .so)."""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_state_cases as S  # noqa: E402
from tests.gemm_state_cases import (CLEAR_P, CLEAR_SHARE, COL_PART_REL, F32, GEMM_REL_L2, NN, NT, SE_DP_REL,  # noqa: E402
                                    SQ_REL, TN, gemm_state)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from mmvae_amd import ops as _ops, _lib

    assert _lib.load().mmvae_abi_version() >= 5
    yield _ops
    for cached in (_gemm_data, _laid_out, recon_data, uncapped_gemm):  # the shared references leave with the module
        cached.cache_clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def state_is_restored():
    yield
    S.assert_default_state()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def asym(m, n):
    """Asymmetric integer-valued matrix (test_kernels_gpu._asym): catches row/col swaps and k-permutation mismatches
    exactly -- every bf16 piece, every product and every partial sum is exact."""
    i = torch.arange(m, dtype=torch.float32).unsqueeze(1)
    j = torch.arange(n, dtype=torch.float32).unsqueeze(0)
    return ((3 * i + 5 * j) % 7) - 3.0 + ((i * j) % 3)


def padded(t, slack=32):
    """engine-style buffer (test_planes_gpu.padded): zero slack rows behind the matrix -- the 16 readable bytes behind a
    rows-contiguous operand that MMVAE_GEMM_OPERAND_SLACK vouches for"""
    full = torch.zeros(t.shape[0] + slack, t.shape[1], device=t.device)
    full[: t.shape[0]] = t
    return full[: t.shape[0]]


def rel(out, ref):
    """rel-L2 against an fp64 reference, on the device"""
    ref = ref.double()
    return float((out.double() - ref).norm() / ref.norm())


# ------------------------------------------------------------------------------------------- shared fp64 references
def gemm_data(M, N, K, scale_b=1.0):
    return _gemm_data(M, N, K, scale_b)


@functools.lru_cache(maxsize=None)
def _gemm_data(M, N, K, scale_b):
    a, b, bias, c0 = rnd(M, K, seed=1), rnd(K, N, seed=2, scale=scale_b), rnd(N, seed=3), rnd(M, N, seed=4)
    ai, bi = asym(M, K), asym(K, N) + 1.0
    d = types.SimpleNamespace(M=M, N=N, K=K)
    d.prod = (a.double() @ b.double()).cuda()        # the reference: fp64 products on the CPU
    d.iprod = (ai.double() @ bi.double()).cuda()
    d.a, d.b, d.ai, d.bi, d.bias, d.c0 = (t.cuda() for t in (a, b, ai, bi, bias, c0))
    return d


def laid_out(M, N, K, layout, integer, scale_b=1.0):
    """(A, B) as the layout wants them; rows-contiguous operands sit in front of zero slack rows"""
    return _laid_out(M, N, K, layout, integer, scale_b)


@functools.lru_cache(maxsize=None)
def _laid_out(M, N, K, layout, integer, scale_b):
    d = gemm_data(M, N, K, scale_b)
    a, b = (d.ai, d.bi) if integer else (d.a, d.b)
    A = a if layout != TN else padded(a.t().contiguous())
    B = b.t().contiguous() if layout == NT else padded(b)
    return A, B


def raw_gemm(layout, A, B, M, N, K, *, out=None, bias=None, alpha=1.0, flags=0, sq_capacity=0):
    """mmvae_gemm_planes_f32 without planes = mmvae_gemm_f32 / _f32_sq with every flag the header has (the wrappers leave
    out bias / ReLU beside MMVAE_GEMM_OPERAND_SLACK and a partial capacity of the caller's choice)."""
    from mmvae_amd import _lib

    lib = _lib.load()
    out = torch.empty(M, N, device="cuda") if out is None else out
    parts = torch.full((sq_capacity,), float("nan"), device="cuda") if sq_capacity else None
    rc = lib.mmvae_gemm_planes_f32(layout, M, N, K, alpha, A.data_ptr(), A.stride(0), None, 0, 0, B.data_ptr(), B.stride(0),
                                   None, 0, 0, out.data_ptr(), out.stride(0), None if bias is None else bias.data_ptr(),
                                   flags, 1, None, 0, None if parts is None else parts.data_ptr(), sq_capacity,
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mmvae_gemm_planes_f32")
    return out, parts


def check_gemm(ops, layout, M, N, K, count, planned=None, slack=False):
    """One unsplit GEMM shape under the current state: exact on integers, the fp64 bound with bias / ReLU / alpha and
    accumulate, the fused norm.  `count`: tiles of the kernel the case names; `planned`: what mmvae_gemm_sq_partials
    answers (larger for a shape that needs operand slack).  Returns (plain output, partials) for bitwise comparisons."""
    from mmvae_amd import _lib

    lib = _lib.load()
    planned = count if planned is None else planned
    assert lib.mmvae_gemm_sq_partials(layout, M, N, K, 0) == planned, "the case does not reach the kernel it names"
    d = gemm_data(M, N, K)
    SLACK = _lib.GEMM_OPERAND_SLACK if slack else 0

    def gemm(A, B, **kw):
        if not slack:
            return ops.gemm(layout, A, B, splitk=1, **kw)
        if not kw or set(kw) <= {"out", "accumulate"}:
            return ops.gemm_planes(layout, A, B, splitk=1, operand_slack=True, **kw)
        flags = SLACK | (_lib.GEMM_RELU if kw.get("relu") else 0) | (_lib.GEMM_ACCUMULATE if kw.get("accumulate") else 0)
        return raw_gemm(layout, A, B, M, N, K, out=kw.get("out"), bias=kw.get("bias"), alpha=kw.get("alpha", 1.0),
                        flags=flags)[0]

    Ai, Bi = laid_out(M, N, K, layout, True)
    out = gemm(Ai, Bi)
    assert torch.equal(out.double(), d.iprod), f"max err {(out.double() - d.iprod).abs().max()}"
    A, B = laid_out(M, N, K, layout, False)
    plain = gemm(A, B)
    assert rel(plain, d.prod) <= GEMM_REL_L2
    with_bias = d.prod + d.bias.double()
    assert rel(gemm(A, B, bias=d.bias), with_bias) <= GEMM_REL_L2
    assert rel(gemm(A, B, bias=d.bias, relu=True), with_bias.clamp_min(0)) <= GEMM_REL_L2
    if slack:  # (through the wrapper the issue names: alpha = 1)
        assert rel(gemm(A, B, out=d.c0.clone(), accumulate=True), d.prod + d.c0.double()) <= GEMM_REL_L2
    out = gemm(A, B, out=d.c0.clone(), alpha=-0.5, accumulate=True)
    assert rel(out, -0.5 * d.prod + d.c0.double()) <= GEMM_REL_L2
    # fused norm: the launch takes exactly the planned count
    if slack:
        out_sq, parts = ops.gemm_planes(layout, A, B, want_sq=True, operand_slack=True)
    else:
        out_sq, parts = ops.gemm_sq(layout, A, B)
    assert parts.numel() == planned
    assert torch.equal(out_sq, plain), "the fused-norm launch stores another product"
    total, want = float(parts.double().sum()), float((plain.double() ** 2).sum())
    assert abs(total - want) <= SQ_REL * want, (total, want)
    assert bool((parts[:count] > 0).all()) and bool((parts[count:] == 0).all()), "one partial per tile of the named kernel"
    # ... and a larger capacity: the same partials, zeros behind them, bitwise again on a second call
    for _ in range(2):
        out_big, big = raw_gemm(layout, A, B, M, N, K, flags=SLACK, sq_capacity=planned + 37)
        assert torch.equal(out_big, plain) and torch.equal(big[:planned], parts)
        assert bool((big[planned:] == 0).all())
    return plain, parts


# ------------------------------------------------------------------------------------- fused reconstruction, shared
@functools.lru_cache(maxsize=None)
def recon_data(R, B, G, H):
    h, W, bias = rnd(R, H, seed=1), rnd(G, H, seed=2, scale=0.2), rnd(G, seed=3, scale=0.1)
    x = rnd(B, G, seed=4).abs()
    d = types.SimpleNamespace()
    P = h.double() @ W.double().t() + bias.double()  # fp64 on the CPU
    d.clear_share = float((P.abs() > CLEAR_P).double().mean())
    d.P = P.cuda()
    d.h, d.W, d.bias, d.x = (t.cuda() for t in (h, W, bias, x))
    d.xh = d.P.clamp_min(0)
    d.d = d.xh - d.x.double().repeat(R // B, 1)
    return d


def check_recon(ops, R, B, G, H, nt):
    """Everything test_kernels_gpu.test_decoder_recon asserts, under the current state; `nt`: column tiles of the kernel
    the case names (rows nt .. of se_part are the zero rows).  Returns (xhat, dP, se_part, col_part)."""
    r = recon_data(R, B, G, H)
    # the compared share of dP: P = h . W^T + bias has a standard deviation of 0.2 sqrt(H) >= 1.6, so |P| <= 1e-4 holds
    # for about 2e-4 / (1.6 sqrt(2 pi)) = 5e-5 of the entries
    assert r.clear_share >= CLEAR_SHARE, r.clear_share
    T = ops.recon_tiles(G)
    assert nt <= T
    xhat, dP, se_part = ops.decoder_recon(r.h, r.W, r.bias, r.x)
    assert rel(xhat, r.xh) <= GEMM_REL_L2
    assert se_part.shape == (T, R)
    assert rel(se_part.double().sum(0), (r.d * r.d).sum(1)) <= SE_DP_REL
    assert bool((se_part[:nt] > 0).all()) and bool((se_part[nt:] == 0).all()), "se_part rows of another tiling"
    clear = r.P.abs() > CLEAR_P
    assert float(clear.double().mean()) >= CLEAR_SHARE
    ref_dp = 2 * r.d * (r.P > 0)
    assert rel(dP.double()[clear], ref_dp[clear]) <= SE_DP_REL
    # optional outputs off
    _, _, se2 = ops.decoder_recon(r.h, r.W, r.bias, r.x, want_xhat=False, want_dP=False)
    assert torch.equal(se2, se_part)
    # bias-gradient partials: column sums of the dP it stored, per 128-row tile
    col_part = torch.full((ops.recon_row_tiles(R), G), float("nan"), device="cuda")
    _, dP2, se4 = ops.decoder_recon(r.h, r.W, r.bias, r.x, col_part=col_part)
    assert torch.equal(dP2, dP) and torch.equal(se4, se_part)
    for t in range(col_part.shape[0]):
        assert rel(col_part[t], dP[128 * t:128 * (t + 1)].double().sum(0)) <= COL_PART_REL, t
    # every row of se_part is defined by the call
    poisoned = torch.full((T, R), float("nan"), device="cuda")
    _, _, se3 = ops.decoder_recon(r.h, r.W, r.bias, r.x, want_xhat=False, want_dP=False, se_part=poisoned)
    assert torch.equal(se3, se_part)
    return xhat, dP, se_part, col_part


RECON_BIG = [(512, 512, 20000, 64), (1024, 512, 19996, 64)]  # one batch, and a K-sample form with a ragged last tile

SLAB_M, SLAB_N = 512, 1024


def check_slabs(slabs, K):
    """raw split-K slabs: they sum to the product; with a K tail the last slab is the tail's product alone
    (test_kernels_gpu.test_gemm_raw_slabs_with_k_tail)"""
    d = gemm_data(SLAB_M, SLAB_N, K, 0.05)
    assert rel(slabs.double().sum(0), d.prod) <= GEMM_REL_L2
    if K % 32:
        km = K // 32 * 32
        tail = d.a[:, km:].cpu().double() @ d.b[km:].cpu().double()
        assert rel(slabs[-1], tail.cuda()) <= GEMM_REL_L2


# ============================================================================== 1. the 2 x 4-wave family (x3w = 0)
OFF_CASES = [(c, lay) for c in S.GEMM_CASES + S.ODD_160_CASES for lay in c.layouts]


def _ids(v):
    return repr(v) if isinstance(v, S.Case) else None


@pytest.mark.parametrize("case,layout", OFF_CASES, ids=_ids)
def test_two_by_four_wave_gemm(ops, case, layout):
    """gemm_x3_kernel at chip-filling shapes: the 128x160 / 160x128 tiles (pipelined VEC loader) and the square tile.
    The odd-extent shapes run with MMVAE_GEMM_OPERAND_SLACK over padded() operands: the edge 16-byte group of a
    rows-contiguous operand -- at 52437 on the square tile, at 19997 in rows 128..159 of the 160-row tiles."""
    with gemm_state(x3w=0):
        check_gemm(ops, layout, case.M, case.N, case.K, case.count(0), case.planned_partials(0), case.slack)


@pytest.mark.parametrize("K", [8192, 8200])
@pytest.mark.parametrize("layout", [NT, NN])
def test_two_by_four_wave_raw_slabs(ops, layout, K):
    """the K = G reductions as the 2 x 4-wave family runs them: 16 slices x 32 square tiles (+ the tail slab at 8200)"""
    A, B = laid_out(SLAB_M, SLAB_N, K, layout, False, 0.05)
    with gemm_state(x3w=0):
        slabs = ops.gemm_slabs(layout, A, B)
    assert slabs.shape[0] == 16 + (K % 32 != 0)
    check_slabs(slabs, K)


@pytest.mark.parametrize("R,B,G,H", RECON_BIG)
def test_two_by_four_wave_decoder_recon(ops, R, B, G, H):
    """the fused reconstruction epilogue on the 128x160 tile (x3_tile_for(rows, G, false)): 125 column tiles, rows
    125 .. 156 of se_part written as zeros"""
    with gemm_state(x3w=0):
        check_recon(ops, R, B, G, H, nt=S.ceil_div(G, 160))


def test_families_agree_to_the_fp64_bound(ops):
    """the same call under x3w = 0 and x3w = 1: both within the bound of fp64 (another accumulation split: not bitwise)"""
    c = S.GEMM_CASES[0]
    A, B = laid_out(c.M, c.N, c.K, NT, False)
    d = gemm_data(c.M, c.N, c.K)
    outs = []
    for x3w in (0, 1):
        with gemm_state(x3w=x3w) as lib:
            assert lib.mmvae_gemm_sq_partials(NT, c.M, c.N, c.K, 0) == c.count(x3w)
            outs.append(ops.gemm(NT, A, B, bias=d.bias, splitk=1))
    for out in outs:
        assert rel(out, d.prod + d.bias.double()) <= GEMM_REL_L2


# =========================================================================== 2. the capped persistent grid (x3w = 1)
@functools.lru_cache(maxsize=None)
def uncapped_gemm(M, N, K, layout, slack):
    from mmvae_amd import ops as _ops

    A, B = laid_out(M, N, K, layout, False)
    with gemm_state(x3w=1):
        if slack:
            return _ops.gemm_planes(layout, A, B, want_sq=True, operand_slack=True)
        return _ops.gemm_sq(layout, A, B)


CAPPED = [(c, lay, cap) for c in S.GEMM_CASES for lay in c.layouts for cap in c.caps
          if cap != 1 or (c.M, c.N) in S.CAP1_SHAPES]


@pytest.mark.parametrize("case,layout,cap", CAPPED, ids=_ids)
def test_capped_persistent_gemm(ops, case, layout, cap):
    """gemm_x3w_kernel on a capped grid: the item loop of <= cap workgroups (cap 1: one workgroup walks every item) and
    the tile the planner takes under that cap.  Where the pinned tile is the uncapped one, output and norm partials are
    bit for bit the uncapped launch's ("results do not depend on the cap")."""
    with gemm_state(x3w=1, cap=cap):
        plain, parts = check_gemm(ops, layout, case.M, case.N, case.K, case.count(1, cap), case.planned_partials(1, cap),
                                  case.slack)
    if case.tile(1, cap) == case.on:
        out0, parts0 = uncapped_gemm(case.M, case.N, case.K, layout, case.slack)
        assert torch.equal(plain, out0) and torch.equal(parts, parts0)


@pytest.mark.parametrize("cap", [86, 125])
@pytest.mark.parametrize("pre", ["b", "ab"])
def test_capped_presplit_operands(ops, pre, cap):
    """pre-split operands under a cap (the planes launch passes the capped slots on its own): bitwise the fp32-operand
    launch under the same cap, within the bound of fp64, and -- cap 86 keeps the 160x256 tile -- bitwise the uncapped one"""
    c = next(c for c in S.GEMM_CASES if (c.M, c.N) == (5120, 2048))
    A, B = laid_out(c.M, c.N, c.K, TN, False)  # (K = 64 is whole k-tiles: no padding over the slack rows needed)
    d = gemm_data(c.M, c.N, c.K)
    ap = ops.split_planes(A) if "a" in pre else None
    bp = ops.split_planes(B)
    kw = dict(want_sq=True, operand_slack=True)
    with gemm_state(x3w=1, cap=cap) as lib:
        assert lib.mmvae_gemm_planes_supported(TN, c.M, c.N, c.K, 1, int("a" in pre), 1) == 1
        f32, sq0 = ops.gemm_planes(TN, A, B, **kw)
        pl, sq1 = ops.gemm_planes(TN, A if ap is None else None, None, a_planes=ap, b_planes=bp, **kw)
    assert sq1.numel() == c.count(1, cap)
    assert torch.equal(pl, f32) and torch.equal(sq0, sq1)
    assert rel(pl, d.prod) <= GEMM_REL_L2
    assert abs(float(sq1.double().sum()) / float((pl.double() ** 2).sum()) - 1) <= SQ_REL
    if c.tile(1, cap) == c.on:
        out0, parts0 = uncapped_gemm(c.M, c.N, c.K, TN, False)
        assert torch.equal(pl, out0) and torch.equal(sq1, parts0)


@pytest.mark.parametrize("cap", [86, 128])
def test_capped_prefetch_slabs(ops, cap):
    """the prefetched first product (engine.py: caps 86 / 128): NT raw slabs with A pre-split.  16 slices x 16 tiles of
    256x128 = 256 items at every one of these caps (3 and 2 rounds x 32768 against 224 items of 256x160 in 3 and 2 rounds
    x 40960), so the slabs are bitwise the uncapped launch's."""
    K = 8192
    A, B = laid_out(SLAB_M, SLAB_N, K, NT, False, 0.05)
    ap = ops.split_planes(A)
    with gemm_state(x3w=1):
        base = ops.gemm_slabs(NT, A, B)
    with gemm_state(x3w=1, cap=cap) as lib:
        assert lib.mmvae_gemm_planes_supported(NT, SLAB_M, SLAB_N, K, 0, 1, 0) == 1
        s_f32 = ops.gemm_slabs(NT, A, B)
        s_pl = ops.gemm_planes(NT, None, B, a_planes=ap, raw_slabs=True)
    assert s_pl.shape == base.shape == (16, SLAB_M, SLAB_N)
    assert torch.equal(s_pl, s_f32) and torch.equal(s_f32, base)
    check_slabs(s_pl, K)


def test_capped_decoder_recon(ops):
    """the fused reconstruction launch on 125 workgroups: 250 tiles of 256x160 capped and uncapped (2 rounds x 40960 against
    3 x 32768 for 314 of 256x128), so every output is bitwise the uncapped launch's"""
    R, B, G, H = RECON_BIG[0]
    with gemm_state(x3w=1):
        want = check_recon(ops, R, B, G, H, nt=S.ceil_div(G, 160))
    with gemm_state(x3w=1, cap=125):
        got = check_recon(ops, R, B, G, H, nt=S.ceil_div(G, 160))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ======================================================================================= 3. exact-f32 products
@pytest.mark.parametrize("layout,M,N,K,tile", S.F32_CASES)
def test_exact_f32_gemm(ops, layout, M, N, K, tile):
    """launch_gemm_vec tiles 0 / 1 (NT tile 1: the BK = 16 variant; K = 72 ends inside its fifth k-step)"""
    with gemm_state(precision=F32):
        check_gemm(ops, layout, M, N, K, S.tiles(M, N, tile))


@pytest.mark.parametrize("layout", [NT, NN, TN])
def test_exact_f32_unaligned_strides(ops, layout):
    """test_kernels_gpu.test_gemm_unaligned_strides in exact-f32 mode"""
    M, N, K = 70, 45, 131
    d = gemm_data(M, N, K)
    A = d.a if layout != TN else d.a.t().contiguous()
    Bm = d.b.t().contiguous() if layout == NT else d.b

    def pad(t, extra):  # view with ld = cols + extra
        buf = torch.zeros(t.shape[0], t.shape[1] + extra, device="cuda")
        buf[:, : t.shape[1]] = t
        return buf[:, : t.shape[1]]

    with gemm_state(precision=F32):
        out = ops.gemm(layout, pad(A, 3), pad(Bm, 1))
        outbuf = torch.zeros(M, N + 5, device="cuda")
        ops.gemm(layout, pad(A, 3), pad(Bm, 1), out=outbuf[:, :N])
    assert rel(out, d.prod) <= GEMM_REL_L2
    assert rel(outbuf[:, :N], d.prod) <= GEMM_REL_L2
    assert float(outbuf[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("layout", [NT, NN, TN])
@pytest.mark.parametrize("M,N,K,splitk", [(130, 70, 1000, 5), (512, 1024, 2000, 0)])
def test_exact_f32_split_k(ops, layout, M, N, K, splitk):
    """two split-K cases of test_kernels_gpu.test_gemm_random on the exact-f32 square tile"""
    d = gemm_data(M, N, K)
    A, B = laid_out(M, N, K, layout, False)
    with_bias = d.prod + d.bias.double()
    with gemm_state(precision=F32):
        assert rel(ops.gemm(layout, A, B, bias=d.bias, splitk=splitk), with_bias) <= GEMM_REL_L2
        assert rel(ops.gemm(layout, A, B, bias=d.bias, relu=True, splitk=splitk), with_bias.clamp_min(0)) <= GEMM_REL_L2
        out = ops.gemm(layout, A, B, out=d.c0.clone(), alpha=-0.5, accumulate=True, splitk=splitk)
        assert rel(out, -0.5 * d.prod + d.c0.double()) <= GEMM_REL_L2
        Ai, Bi = laid_out(M, N, K, layout, True)
        assert torch.equal(ops.gemm(layout, Ai, Bi, splitk=splitk).double(), d.iprod)


@pytest.mark.parametrize("K", [8192, 8200])
@pytest.mark.parametrize("layout", [NT, NN])
def test_exact_f32_raw_slabs(ops, layout, K):
    """16 slices of 16 k-tiles on the square tile; at 8200 the planner adds a slab, which then holds k-tile 256 = the
    eight tail columns alone"""
    A, B = laid_out(SLAB_M, SLAB_N, K, layout, False, 0.05)
    with gemm_state(precision=F32):
        slabs = ops.gemm_slabs(layout, A, B)
    assert slabs.shape[0] == 16 + (K % 32 != 0)
    check_slabs(slabs, K)


@pytest.mark.parametrize("R,B,G,H", [(33, 33, 257, 72), (512, 512, 20000, 64), (1024, 512, 19996, 72)])
def test_exact_f32_decoder_recon(ops, R, B, G, H):
    """the fused reconstruction kernel on tile 1 (128x160, BK = 16): se_part has ceil(G / 160) rows, all of them used"""
    with gemm_state(precision=F32):
        assert ops.recon_tiles(G) == S.ceil_div(G, 160)
        check_recon(ops, R, B, G, H, nt=S.ceil_div(G, 160))


def test_exact_f32_refusals_and_fallbacks(ops):
    """pre-split operands have no exact-f32 kernels: planes outputs are refused, planes inputs fall back to the fp32
    operand when one is given (bitwise the plain call) and fail loudly otherwise"""
    from mmvae_amd import _lib

    R, B, G, H = RECON_BIG[0]
    r = recon_data(R, B, G, H)
    hp = ops.split_planes(r.h)
    c = next(c for c in S.GEMM_CASES if (c.M, c.N) == (5120, 2048))
    A, Bm = laid_out(c.M, c.N, c.K, TN, False)
    ap, bp = ops.split_planes(A), ops.split_planes(Bm)
    with gemm_state(precision=F32):
        with pytest.raises(_lib.HipLibraryError, match="MMVAE_ERR_ARG"):
            ops.decoder_recon(r.h, r.W, r.bias, r.x, want_xhat=False, want_dP=False, dP_planes=ops.Planes(R, G, "cuda"))
        want = ops.decoder_recon(r.h, r.W, r.bias, r.x)
        got = ops.decoder_recon(r.h, r.W, r.bias, r.x, h_planes=hp)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert rel(got[0], r.xh) <= GEMM_REL_L2
        ref = ops.gemm(TN, A, Bm)
        assert torch.equal(ops.gemm_planes(TN, A, Bm, a_planes=ap, b_planes=bp), ref)
        assert rel(ref, gemm_data(c.M, c.N, c.K).prod) <= GEMM_REL_L2
        with pytest.raises(_lib.HipLibraryError, match="MMVAE_ERR_ARG"):
            ops.gemm_planes(TN, None, None, a_planes=ap, b_planes=bp)
    torch.cuda.synchronize()  # (the refused calls enqueued nothing that fails later)
