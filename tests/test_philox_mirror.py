"""The host mirror of the Philox kernels (tests/philox_mirror.py) against published known answers: what the GPU tests
compare the kernels with has to be right on its own.  No GPU, no project import."""
import itertools

import numpy as np
import pytest

from tests import philox_mirror as M

# Random123 known-answer vectors for philox4x32-10: counter words c0..c3, key words k0, k1, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers_by_words(ctr, key, want):
    got = M.philox_rounds(*ctr, *key)
    assert tuple(int(g[0]) for g in got) == want


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers_through_the_kernel_word_layout(ctr, key, want):
    """counter = c1:c0, stream = c3:c2, seed = k1:k0 -- and vectorised: the vector sits between two other counters."""
    counter = (ctr[1] << 32) | ctr[0]
    stream, seed = (ctr[3] << 32) | ctr[2], (key[1] << 32) | key[0]
    got = M.philox4x32_10(np.array([5, counter, 7], dtype=np.uint64), stream, seed)
    assert tuple(int(g[1]) for g in got) == want
    assert all(g.dtype == np.uint32 and g.shape == (3,) for g in got)
    assert tuple(int(g[0]) for g in got) != want and tuple(int(g[2]) for g in got) != want


def test_nine_rounds_give_other_numbers():
    for ctr, key, want in KAT:
        assert tuple(int(g[0]) for g in M.philox_rounds(*ctr, *key, rounds=9)) != want


def test_counters_carry_into_the_high_word_and_wrap():
    c = M.counters(16, 2 ** 32 - 2)
    assert [int(v) for v in c] == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    c = M.counters(8, 2 ** 64 - 1)
    assert [int(v) for v in c] == [2 ** 64 - 1, 0]
    w = M.words(16, 9, 2 ** 32 - 2, 3)
    assert w.shape == (4, 4)
    one = M.philox4x32_10(2 ** 32, 3, 9)  # high counter word 1, low 0
    assert [int(v) for v in w[2]] == [int(v[0]) for v in one]
    assert [int(v) for v in w[2]] != [int(v[0]) for v in M.philox4x32_10(0, 3, 9)]


def test_u01_edges_bit_for_bit():
    """k + 0.5f is not representable for k >= 2^23 and rounds to even: the top of the range is exactly 1.0f."""
    k = np.array([0, 2 ** 23, 2 ** 24 - 2, 2 ** 24 - 1], dtype=np.uint32)
    for low in (0, 0xFF):  # the low 8 bits of the word are dropped
        u = M.u01((k << np.uint32(8)) | np.uint32(low))
        assert u.dtype == np.float32
        want = np.array([2.0 ** -25, 0.5, 1.0 - 2.0 ** -23, 1.0], dtype=np.float32)
        assert u.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    every = M.u01(np.arange(0, 2 ** 24, 4099, dtype=np.uint32) << np.uint32(8))
    assert float(every.min()) == 2.0 ** -25 and float(every.max()) <= 1.0 and bool(np.all(np.diff(every) >= 0))


def test_normal_is_finite_at_the_extreme_words():
    combos = np.array(list(itertools.product([0, 0xFFFFFFFF], repeat=4)), dtype=np.uint32)
    vals, radii = M.normal_from_words(combos)
    assert vals.shape == (16, 4) and bool(np.isfinite(vals).all()) and bool(np.isfinite(radii).all())
    # u0 == 1.0f: radius exactly zero, both outputs zero; u0 == 2^-25: the largest radius
    assert bool(np.all(radii[combos[:, 0] == 0xFFFFFFFF, 0] == 0)) and bool(np.all(vals[combos[:, 0] == 0xFFFFFFFF, :2] == 0))
    assert abs(float(radii.max()) - float(np.sqrt(50.0 * np.log(2.0)))) < 1e-12


def test_fills_are_prefixes_and_layouts_agree():
    seed, off, stream = 1234, 2 ** 32 - 3, 2 ** 32 + 7
    w = M.words(21, seed, off, stream)
    assert w.shape == (6, 4)
    m = M.keep_mask(21, 0.5, seed, off, stream)
    assert m.dtype == np.uint8 and m.shape == (21,)
    assert m.tolist() == (M.u01(w).reshape(-1)[:21] >= np.float32(0.5)).astype(int).tolist()
    assert M.keep_mask(7, 0.5, seed, off, stream).tolist() == m[:7].tolist()
    assert M.keep_mask(21, 0.0, seed, off, stream).all() and M.keep_mask(21, 2.0 ** -25, seed, off, stream).all()
    v = M.normal(21, seed, off, stream)
    assert v.dtype == np.float64 and v.shape == (21,)
    v2, r2 = M.normal_with_radius(9, seed, off + 1, stream)
    assert v2.tolist() == v[4:13].tolist()
    # value pairs lie on the circle of their radius
    assert np.allclose(np.hypot(v2[0], v2[1]), r2[0], rtol=1e-12) and r2[0] == r2[1] and r2[2] == r2[3]


def test_normal_moments():
    v = M.normal(200000, 77, 5, 0x4E4F524D)
    assert abs(v.mean()) < 0.01 and abs(v.std() - 1.0) < 0.01 and abs((v ** 4).mean() - 3.0) < 0.1
