"""Host-only half of the launch-state tests: every case of tests/gemm_state_cases.py reaches the kernel it names.

mmvae_gemm_sq_partials is the planner's own answer to "how many tiles does the unsplit launch of this shape have" under
the current (kernel family, precision, cap): equal to ceil(M / bm) * ceil(N / bn) of the pinned tile, it pins the tile
family without a device (the library loads on a host without a GPU and plans for 256 compute units there)."""
import os

import pytest

from tests import gemm_state_cases as S
from tests.gemm_state_cases import BF16X3, F32, NN, NT, TN, gemm_state

ALL_CASES = S.GEMM_CASES + S.ODD_160_CASES
SHAPE_LAYOUT = [(c, lay) for c in ALL_CASES for lay in c.layouts]


@pytest.fixture(autouse=True)
def state_is_restored():
    yield
    S.assert_default_state()


def _ids(v):
    return repr(v) if isinstance(v, S.Case) else None


@pytest.mark.parametrize("case,layout", SHAPE_LAYOUT, ids=_ids)
def test_two_by_four_wave_family_tiles(case, layout):
    """x3w = 0: the 2 x 4-wave bf16x3 kernels (tile ids 3 / 4 / 5)."""
    with gemm_state(x3w=0) as lib:
        assert lib.mmvae_gemm_get_x3w() == 0
        assert lib.mmvae_gemm_sq_partials(layout, case.M, case.N, case.K, 0) == case.planned_partials(0)
        if case.twin:
            assert lib.mmvae_gemm_sq_partials(layout, *case.twin, case.K, 0) == case.count(0)
        # a cap is the persistent kernel's: it does not reach this family
        assert lib.mmvae_gemm_set_workgroup_cap(125) == 0
        assert lib.mmvae_gemm_sq_partials(layout, case.M, case.N, case.K, 0) == case.planned_partials(0)


@pytest.mark.parametrize("case,layout", SHAPE_LAYOUT, ids=_ids)
def test_persistent_kernel_tiles_uncapped_and_capped(case, layout):
    """x3w = 1: tile ids 6 / 7 / 8, costed over the capped slots.  Every cap the GPU tests use, the engine's own caps
    (125, 185, 170, 86, 128: engine.py:45-61) and the no-op caps (0, >= the device's compute units)."""
    seen = set()
    with gemm_state(x3w=1) as lib:
        for cap in (0, 1, 86, 125, 128, 170, 185, 255, 256, 300, 1 << 20):
            assert lib.mmvae_gemm_set_workgroup_cap(cap) == 0
            got = lib.mmvae_gemm_sq_partials(layout, case.M, case.N, case.K, 0)
            assert got == case.planned_partials(1, cap), (cap, got)
            if case.twin:
                assert lib.mmvae_gemm_sq_partials(layout, *case.twin, case.K, 0) == case.count(1, cap), cap
            if cap == 0 or cap >= 256:  # a cap of 256 or more gives the uncapped counts
                assert got == case.planned_partials(1, 0)
            seen.add(case.tile(1, cap))
    assert case.on in seen and (not case.capped or len(seen) > 1)


def test_the_table_covers_every_tile_of_both_families():
    off = {c.off for c in ALL_CASES}
    on = {c.tile(1, cap) for c in ALL_CASES for cap in (0,) + tuple(c.caps)}
    assert off == {S.T128, S.T128x160, S.T160x128} and on == {S.W256x160, S.W160x256, S.W256x128}
    for c in S.GEMM_CASES:  # each shape of the table meets a cap that changes its tile and one that keeps it
        tiles_capped = {c.tile(1, cap) for cap in c.caps}
        assert c.on in tiles_capped and len(tiles_capped) > 1, c


@pytest.mark.parametrize("layout,M,N,K,tile", S.F32_CASES)
def test_exact_f32_tiles(layout, M, N, K, tile):
    """MMVAE_GEMM_PRECISION_F32: plan()'s own tiles 0 / 1 (launch_gemm_vec), whatever the family switch and the cap say."""
    for x3w, cap in ((-1, 0), (0, 0), (1, 125)):
        with gemm_state(x3w=x3w, precision=F32, cap=cap) as lib:
            assert lib.mmvae_gemm_get_precision() == F32
            assert lib.mmvae_gemm_sq_partials(layout, M, N, K, 0) == S.tiles(M, N, tile)


def test_exact_f32_has_no_planes_kernels_and_160_wide_recon_tiles():
    with gemm_state(precision=F32) as lib:
        for layout, M, N, K, pa, pb in ((TN, 2048, 5120, 512, 1, 1), (TN, 5120, 2048, 64, 0, 1), (NT, 512, 1024, 20000, 1, 0),
                                        (NN, 512, 1024, 20000, 1, 0)):
            assert lib.mmvae_gemm_planes_supported(layout, M, N, K, 0, pa, pb) == 0
        assert lib.mmvae_recon_tiles(20000) == 125 and lib.mmvae_recon_tiles(257) == 2 and lib.mmvae_recon_tiles(19996) == 125
    lib = S._load()
    assert lib.mmvae_gemm_planes_supported(TN, 2048, 5120, 512, 0, 1, 1) == 1  # (the same question in the default mode)
    assert lib.mmvae_recon_tiles(20000) == 157


def test_planes_support_follows_family_and_cap():
    """Pre-split operands exist on the persistent kernel only; the capped cases the GPU tests run are supported."""
    with gemm_state(x3w=0) as lib:
        assert lib.mmvae_gemm_planes_supported(TN, 5120, 2048, 64, 1, 1, 1) == 0
    for cap in (0, 86, 125):
        with gemm_state(x3w=1, cap=cap) as lib:
            assert lib.mmvae_gemm_planes_supported(TN, 5120, 2048, 64, 1, 1, 1) == 1
            assert lib.mmvae_gemm_planes_supported(TN, 5120, 2048, 64, 1, 0, 1) == 1
    for cap in (0, 86, 128):  # the prefetched first product: 16 raw slabs of 512 x 1024, A pre-split
        with gemm_state(x3w=1, cap=cap) as lib:
            assert lib.mmvae_gemm_planes_supported(NT, 512, 1024, 8192, 0, 1, 0) == 1


def test_workgroup_cap_argument():
    from mmvae_amd import _lib

    with gemm_state(x3w=1, cap=125) as lib:
        assert lib.mmvae_gemm_sq_partials(*S.SENTINEL, 0) == 320
        assert lib.mmvae_gemm_set_workgroup_cap(-1) == _lib.ERR_ARG
        assert lib.mmvae_gemm_sq_partials(*S.SENTINEL, 0) == 320  # the refused call left the cap as it was
        assert lib.mmvae_gemm_set_x3w(2) == _lib.ERR_ARG and lib.mmvae_gemm_set_x3w(-2) == _lib.ERR_ARG
        assert lib.mmvae_gemm_get_x3w() == 1


def test_family_switch_wins_over_the_environment():
    """mmvae_gemm_set_x3w(0 / 1) decides whatever MMVAE_X3W says; -1 follows the variable (read at every launch)."""
    lib = S._load()
    before = os.environ.get("MMVAE_X3W")
    try:
        for env, follows in (("0", 0), ("1", 1), (None, 1)):
            if env is None:
                os.environ.pop("MMVAE_X3W", None)
            else:
                os.environ["MMVAE_X3W"] = env
            for mode, want in ((0, 0), (1, 1), (-1, follows)):
                with gemm_state(x3w=mode):
                    assert lib.mmvae_gemm_get_x3w() == want, (env, mode)
                    assert lib.mmvae_gemm_sq_partials(*S.SENTINEL, 0) == (256 if want else 512), (env, mode)
            assert lib.mmvae_gemm_get_x3w() == follows  # gemm_state went back to -1
    finally:
        if before is None:
            os.environ.pop("MMVAE_X3W", None)
        else:
            os.environ["MMVAE_X3W"] = before


def test_state_context_restores_after_an_exception():
    lib = S._load()
    with pytest.raises(RuntimeError):
        with gemm_state(x3w=0, precision=F32, cap=86):
            assert (lib.mmvae_gemm_get_x3w(), lib.mmvae_gemm_get_precision()) == (0, F32)
            raise RuntimeError("boom")
    assert lib.mmvae_gemm_get_precision() == BF16X3
