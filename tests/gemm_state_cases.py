"""Launch states of the chip-filling GEMMs and of the fused reconstruction kernel, and the cases the two
test_gemm_launch_state* files run under them.

Three process-wide switches decide which kernel a call runs (include/mmvae_hip.h): mmvae_gemm_set_x3w (kernel family:
wave-specialised persistent kernel or the 2 x 4-wave kernels), mmvae_gemm_set_precision (bf16x3 or exact-f32 products)
and mmvae_gemm_set_workgroup_cap (grid of the persistent kernel; the planner costs its tiles over the capped slots, so a
cap can change the tile shape).  `gemm_state` sets all three and always restores the defaults.

The tile tables are pinned by hand from plan / x3_tile_for / x3w_tile_for (mmvae_amd/csrc/gemm_f32.hip) for a
256-CU device -- also what the library assumes on a host without a GPU: cost of a tile shape = rounds of the
resident-workgroup slots x tile area, first candidate wins a tie.  The host-only test holds the library to them through
mmvae_gemm_sq_partials (= tiles of the unsplit launch); the GPU tests repeat that check on the device before they launch.

Plain module: nothing here touches a device when it is imported."""
import contextlib
import os

NT, NN, TN = 0, 1, 2
F32, BF16X3 = 0, 1  # MMVAE_GEMM_PRECISION_*

# The project's own bounds, each with the line that sets it.
GEMM_REL_L2 = 2e-6   # tests/test_kernels_gpu.py:3   GEMM outputs and xhat, rel-L2 against fp64 (bf16x3 and exact f32 alike)
SQ_REL = 1e-5        # tests/test_kernels_gpu.py:792 sum of the fused norm partials against the fp64 sum of squares
SE_DP_REL = 1e-5     # tests/test_kernels_gpu.py:194,198  se_part sums and dP (where |P| > 1e-4)
COL_PART_REL = 1e-6  # tests/test_kernels_gpu.py:208 col_part per 128-row tile
CLEAR_P = 1e-4       # tests/test_kernels_gpu.py:197 entries of dP that are compared: |P| beyond rounding of the ReLU edge
CLEAR_SHARE = 0.99   # ... and the least share of the entries they must be

CAPS = (1, 86, 125, 185, 255)

# tile shapes by kernel family (tile ids of gemm_f32.hip)
T128, T128x160, T160x128 = (128, 128), (128, 160), (160, 128)   # 2 x 4-wave bf16x3 (3, 4, 5) / exact f32 (0, 1)
W256x160, W160x256, W256x128 = (256, 160), (160, 256), (256, 128)  # wave-specialised (6, 7, 8)


def ceil_div(a, b):
    return -(-a // b)


def tiles(M, N, tile):
    return ceil_div(M, tile[0]) * ceil_div(N, tile[1])


class Case:
    """One output shape: the tile each state takes.  `capped` maps a cap to its tile; caps it does not list keep the
    uncapped tile.  `twin`: a rows-contiguous extent off a multiple of 4 reaches the pipelined kernels only when the
    caller vouches for slack behind the operands, which mmvae_gemm_sq_partials cannot know -- it then answers the larger
    of the pipelined and the element-guarded (128x128) count.  The planner's choice for such a shape is pinned on its
    16-byte-regular twin (same tile counts for every candidate shape)."""

    def __init__(self, layouts, M, N, K, off, on, capped=None, caps=CAPS, twin=None):
        self.layouts, self.M, self.N, self.K = layouts, M, N, K
        self.off, self.on, self.capped, self.caps, self.twin = off, on, dict(capped or {}), caps, twin

    @property
    def slack(self):
        return self.twin is not None

    def tile(self, x3w, cap=0):
        if not x3w:
            return self.off
        return self.capped.get(cap, self.on) if 0 < cap < 256 else self.on

    def count(self, x3w, cap=0):
        return tiles(self.M, self.N, self.tile(x3w, cap))

    def planned_partials(self, x3w, cap=0):
        """what mmvae_gemm_sq_partials answers for the shape itself"""
        n = self.count(x3w, cap)
        return max(n, tiles(self.M, self.N, T128)) if self.slack else n

    def __repr__(self):
        return f"{self.M}x{self.N}x{self.K}"


# K = 64: two k-tiles, the smallest reduction that runs the pipelined loop's steady state and its last tile.
GEMM_CASES = [
    # 512 x 20000: 500 tiles of 128x160 fill the 512 slots of the 2 x 4-wave kernel in one round (628 square ones need
    # two); 250 of 256x160 fill the 256 slots of the persistent kernel in one round.  Caps 170 / 185: 250 tiles and 314
    # of 256x128 both take two rounds, the smaller tile is cheaper.  Caps 1, 86, 125, 255: 256x160 stays cheaper.
    Case((NT, NN, TN), 512, 20000, 64, T128x160, W256x160, {170: W256x128, 185: W256x128}),
    Case((NT, TN), 20000, 512, 64, T160x128, W160x256, {170: W256x128, 185: W256x128}),
    # 2048 x 5120: 256 tiles of 256x160 = one round uncapped; under caps 125, 185 and 255 they take 3, 2 and 2 rounds,
    # as many as the 320 tiles of 256x128.  Caps 1 and 86: 256 x 40960 < 320 x 32768 and 3 x 40960 < 4 x 32768.
    Case((TN,), 2048, 5120, 64, T128x160, W256x160, {125: W256x128, 170: W256x128, 185: W256x128, 255: W256x128}),
    Case((TN,), 5120, 2048, 64, T160x128, W160x256, {125: W256x128, 170: W256x128, 185: W256x128, 255: W256x128}),
    # 4096 x 4096: 512 tiles of 256x128 = two rounds uncapped (416 of 256x160 too, at a larger area); caps 125 and 255
    # bring 256x160 down to 4 and 2 rounds against 5 and 3 (cap 125 is a tie in cost: the first candidate wins).
    Case((TN,), 4096, 4096, 64, T128, W256x128, {125: W256x160, 170: W256x160, 255: W256x160}),
    # The mouse gene count (odd): 2 x 4-wave family 3280 square tiles = 7 rounds x 16384 against 2624 of 128x160 = 6
    # rounds x 20480; persistent kernel 1640 tiles of 256x128 = 7 rounds x 32768 against 1312 of 256x160 = 6 x 40960.
    # Cap 125: 11 rounds x 40960 against 14 x 32768.
    Case((TN,), 1024, 52437, 64, T128, W256x128, {1: W256x160, 86: W256x160, 125: W256x160, 170: W256x160},
         caps=(125, 255), twin=(1024, 52440)),
    Case((TN,), 52437, 1024, 64, T128, W256x128, {1: W160x256, 86: W160x256, 125: W160x256, 170: W160x256},
         caps=(125, 255), twin=(52440, 1024)),
]
CAP1_SHAPES = {(512, 20000), (2048, 5120)}  # one workgroup loops over every item

# Odd rows-contiguous extents ON the 160-row tiles of the 2 x 4-wave family (the 52437-wide shapes plan the square tile
# there): the edge 16-byte group of a row sits in rows 128..159 of the last tile, the DPP-transposed unit.
ODD_160_CASES = [
    Case((TN,), 512, 19997, 64, T128x160, W256x160, {170: W256x128, 185: W256x128}, twin=(512, 20000)),
    Case((TN,), 19997, 512, 64, T160x128, W160x256, {170: W256x128, 185: W256x128}, twin=(20000, 512)),
]

# exact-f32 mode: plan()'s tiles 0 (128x128) / 1 (128x160; no NN form), (layout, M, N, K, tile)
F32_CASES = [
    (NT, 512, 20000, 64, T128x160),
    (NN, 512, 20000, 64, T128),
    (TN, 512, 20000, 64, T128x160),
    (TN, 20000, 512, 64, T128),      # 628 tiles either way = two rounds: the square tile is smaller
    (NT, 512, 20000, 72, T128x160),  # K off the NT tile's 16-wide k-step
    (NN, 512, 20000, 72, T128),
    (TN, 512, 20000, 72, T128x160),
]

# the shape every test asks for after it restored the state: 256 tiles of 256x160 uncapped (320 under cap 125, 512 of
# 128x160 with the persistent kernel off)
SENTINEL = (TN, 2048, 5120, 64)


def env_x3w():
    e = os.environ.get("MMVAE_X3W")
    return 0 if (e and e[0] == "0") else 1


def _load():
    from mmvae_amd import _lib

    return _lib.load()


@contextlib.contextmanager
def gemm_state(x3w=-1, precision=BF16X3, cap=0):
    """Set (kernel family, precision, workgroup cap) for the launches inside; the defaults come back whatever happens."""
    lib = _load()
    try:
        assert lib.mmvae_gemm_set_x3w(x3w) == 0
        assert lib.mmvae_gemm_set_precision(precision) == 0
        assert lib.mmvae_gemm_set_workgroup_cap(cap) == 0
        yield lib
    finally:
        lib.mmvae_gemm_set_x3w(-1)
        lib.mmvae_gemm_set_precision(BF16X3)
        lib.mmvae_gemm_set_workgroup_cap(0)


def assert_default_state():
    """Leaked launch state would corrupt every later test of the process."""
    lib = _load()
    assert lib.mmvae_gemm_get_precision() == BF16X3
    assert lib.mmvae_gemm_get_x3w() == env_x3w()
    want = tiles(SENTINEL[1], SENTINEL[2], W256x160 if env_x3w() else T128x160)
    assert lib.mmvae_gemm_sq_partials(*SENTINEL, 0) == want
