"""mmvae_stats_row_corr_f32 on the GPU: corrcoef of the rows of a stacked (cis ; cross) pair and its block means against
fp64 np.corrcoef of the same fp32 inputs.

Bound (worst case, derived, not measured): every fp32 product chain of the Gram pass is 64 genes long and errs by at
most 64 * 2^-24 * sum |d_i d_j|; by Cauchy-Schwarz the numerator's share of r is at most 64 * 2^-24 and the two diagonal
terms under the root add as much again; fp32 centring adds 2 * 2^-24, the fp32 store 2^-24:
|corr - expected| <= (2 * 64 + 4) * 2^-24 = 7.9e-6 -> 8e-6.  The block means and rel (where cis + cross >= 0.1) are held
to the same figure.  Each test prints the maxima it measured."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 8e-6
# (n_a, n_b, G, mean, sigma, seed).  mean None: ReLU-like values max(noise + shared - shift, 0), many exact zeros.
#   (2, 0, 5)          the smallest accepted shape, no second operand
#   (3, 2, 70)         one partial row block, one whole gene chunk and a 6-gene tail
#   (17, 16, 1030)     mean 1000, sigma 1e-3: ulp(m) is 6 % of the spread, the sd_i sd_j / G correction is decisive
#   (33, 31, 4099)     an odd G, 65 gene chunks = 65 gene splits, a 3-gene tail chunk
#   (100, 100, 260)    R no multiple of 16 (nor of the 128-row block): two row blocks, three block pairs
#   (257, 255, 131)    4 row blocks, 10 block pairs, the a / b boundary inside a block
#   (1100, 948, 67)    R = 2048, the cap: 136 block pairs, one split
# The seeds are those for which every fp64 block mean lies >= 1e-4 from a x.xxx5 rounding boundary (test_rounding
# asserts it: a condition on the inputs).
CASES = [(2, 0, 5, None, 1.0, 0), (3, 2, 70, None, 1.0, 2), (17, 16, 1030, 1000.0, 1e-3, 1), (33, 31, 4099, None, 1.0, 3),
         (100, 100, 260, None, 1.0, 9), (257, 255, 131, None, 1.0, 0), (1100, 948, 67, None, 1.0, 13)]
IDS = [f"{c[0]}+{c[1]}x{c[2]}" for c in CASES]


def make_inputs(n_a, n_b, G, mean, sigma, seed):
    rng = np.random.default_rng(1000 + seed)
    R = n_a + n_b
    shared = rng.standard_normal(G)
    if mean is None:
        x = np.maximum(rng.standard_normal((R, G)) + 0.9 * shared - 0.5, 0.0)
        x[n_a:] = np.maximum(x[n_a:] + 0.6 * rng.standard_normal((n_b, G)) - 0.1, 0.0)
    else:
        x = mean + sigma * (rng.standard_normal((R, G)) + 0.9 * shared)
    x = x.astype(np.float32)
    x[n_a // 2] = 0.0  # an all-zero row in a
    if n_b:
        x[n_a + n_b // 2] = np.float32(3.1415927)  # a constant non-zero row in b
    return x[:n_a].copy(), x[n_a:].copy()


_expected_cache = {}


def expected(a, b, key=None):
    """(corr, [cis, cross, comb, rel], [constant rows of a, of b]) in fp64 from the fp32 inputs, as the reference forms
    them: np.corrcoef of the stacked rows, nan_to_num block means."""
    if key is not None and key in _expected_cache:
        return _expected_cache[key]
    n = a.shape[0]
    x = np.vstack([a, b]).astype(np.float64) if b is not None and b.shape[0] else a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.corrcoef(x)
        z = np.nan_to_num(c)
        cis = z[:n, :n].mean()
        cross = z[n:, n:].mean() if x.shape[0] > n else np.nan
        comb = z[:n, n:].mean() if x.shape[0] > n else np.nan
        rel = 2 * comb / (cis + cross)
    const = (x == x[:, :1]).all(1)
    out = (c, np.array([cis, cross, comb, rel]), [int(const[:n].sum()), int(const[n:].sum())])
    if key is not None:
        _expected_cache[key] = out
    return out


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def check(corr, stats, want, what):
    want_c, want_s, want_n = want
    s = stats.cpu().numpy()
    assert s.shape == (8,) and s.dtype == np.float64
    assert s[4:].tolist() == [float(want_n[0]), float(want_n[1]), 0.0, 0.0], (what, s[4:])
    assert np.array_equal(np.isnan(s[:4]), np.isnan(want_s)), (what, s[:4], want_s)
    have = ~np.isnan(want_s[:3])
    err_s = float(np.abs(s[:3][have] - want_s[:3][have]).max())
    print(f"{what}: max |mean - expected| {err_s:.3g}")
    assert err_s <= BOUND, (what, err_s)
    if not np.isnan(want_s[3]) and want_s[0] + want_s[1] >= 0.1:
        err_rel = abs(float(s[3]) - float(want_s[3]))
        print(f"{what}: |rel - expected| {err_rel:.3g}")
        assert err_rel <= BOUND, (what, err_rel)
    if corr is None:
        return
    got = corr.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want_c.shape
    assert np.array_equal(np.isnan(got), np.isnan(want_c)), f"{what}: NaN positions differ"
    ok = ~np.isnan(want_c)
    err = float(np.abs(got.astype(np.float64)[ok] - want_c[ok]).max())
    print(f"{what}: max |corr - expected| {err:.3g} over {int(ok.sum())} entries, {int((~ok).sum())} NaN")
    assert err <= BOUND, (what, err)
    assert (np.abs(got[ok]) <= 1.0).all()
    live = ~np.isnan(np.diag(want_c))
    assert (np.diag(got)[live] == np.float32(1.0)).all(), f"{what}: diagonal"
    assert np.array_equal(got.view(np.int32), got.T.view(np.int32)), f"{what}: not bitwise symmetric"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from mmvae_amd import ops as _ops

    return _ops


def dev(m):
    return None if m is None or m.shape[0] == 0 else torch.from_numpy(m).cuda()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_accuracy_nan_rule_symmetry_and_reproducibility(ops, case):
    a, b = make_inputs(*case)
    want = expected(a, b, key=case)
    assert want[2] == [1, 1 if case[1] else 0]
    ta, tb = dev(a), dev(b)
    corr, stats = ops.row_corrcoef(ta, tb)
    check(corr, stats, want, IDS[CASES.index(case)])
    again, stats_again = ops.row_corrcoef(ta, tb)
    assert torch.equal(bits(again), bits(corr)) and torch.equal(bits(stats_again), bits(stats))
    none, stats_only = ops.row_corrcoef(ta, tb, want_matrix=False)  # no matrix: the same stats, bit for bit
    assert none is None and torch.equal(bits(stats_only), bits(stats))
    out = torch.full((corr.shape[0], corr.shape[0] + 3), 7.0, device="cuda")
    got, _ = ops.row_corrcoef(ta, tb, out=out[:, :corr.shape[0]])
    assert got.data_ptr() == out.data_ptr() and torch.equal(bits(got), bits(corr)) and (out[:, corr.shape[0]:] == 7.0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounding(ops, case):
    """The means rounded to 3 decimals equal the fp64 ones rounded (what the reference reports)."""
    a, b = make_inputs(*case)
    _, want_s, _ = expected(a, b, key=case)
    means = want_s[:3][~np.isnan(want_s[:3])]
    frac = np.abs(means * 1000.0 - np.floor(means * 1000.0) - 0.5)
    assert (frac >= 0.1).all(), f"inputs: a mean lies within 1e-4 of a rounding boundary ({means}); choose another seed"
    _, stats = ops.row_corrcoef(dev(a), dev(b), want_matrix=False)
    got = stats.cpu().numpy()[:3][~np.isnan(want_s[:3])]
    assert np.array_equal(np.round(got, 3), np.round(means, 3)), (got, means)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_two_operands_equal_stacked(ops, case):
    a, b = make_inputs(*case)
    x = np.vstack([a, b])
    base, _ = ops.row_corrcoef(dev(a), dev(b))
    stacked, stats = ops.row_corrcoef(dev(x), None)
    assert torch.equal(bits(stacked), bits(base))
    assert np.isnan(stats.cpu().numpy()[1:4]).all()
    for cut in (1, x.shape[0] // 3, x.shape[0] - 1):
        other, _ = ops.row_corrcoef(dev(x[:cut]), dev(x[cut:]))
        assert torch.equal(bits(other), bits(base)), cut


def test_strides_and_alignment(ops):
    case = CASES[4]
    n_a, n_b, G = case[:3]
    a, b = make_inputs(*case)
    ta, tb = dev(a), dev(b)
    assert ta.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0 and G % 4 == 0
    base, base_stats = ops.row_corrcoef(ta, tb)
    check(base, base_stats, expected(a, b, key=case), "contiguous, 16-byte rows")

    def widened(m, ld):
        buf = torch.full((m.shape[0], ld), -5.0, device="cuda")
        buf[:, :G] = torch.from_numpy(m).cuda()
        return buf[:, :G]

    def shifted(m):
        flat = torch.zeros(m.size + 1, device="cuda")
        flat[1:] = torch.from_numpy(m).cuda().flatten()
        view = flat[1:].view(m.shape)
        assert view.data_ptr() % 16 == 4
        return view

    variants = {
        "ld a multiple of 4": (widened(a, G + 8), widened(b, G + 4)),
        "ld no multiple of 4": (widened(a, G + 3), widened(b, G + 1)),
        "base one float off": (shifted(a), shifted(b)),
        "a aligned, b not": (ta, shifted(b)),
        "a not, b aligned": (widened(a, G + 5), tb),
    }
    for what, (va, vb) in variants.items():
        corr, stats = ops.row_corrcoef(va, vb)
        assert torch.equal(bits(corr), bits(base)) and torch.equal(bits(stats), bits(base_stats)), what
    # a narrower view: the last 4-gene group straddles the end of the row
    narrow, narrow_stats = ops.row_corrcoef(ta[:, :G - 1], tb[:, :G - 1])
    check(narrow, narrow_stats, expected(a[:, :G - 1], b[:, :G - 1]), "[:, :G - 1] views")
    off, off_stats = ops.row_corrcoef(shifted(a[:, :G - 1].copy()), shifted(b[:, :G - 1].copy()))
    assert torch.equal(bits(off), bits(narrow)) and torch.equal(bits(off_stats), bits(narrow_stats))


def test_argument_checks_launch_nothing(ops):
    from mmvae_amd import _lib, _stats_lib

    lib = _stats_lib.load_stats()
    n_a, n_b, G = 5, 4, 12
    R = n_a + n_b
    a, b = torch.rand(n_a, G, device="cuda"), torch.rand(n_b, G, device="cuda")
    need = lib.mmvae_stats_row_corr_workspace_bytes(n_a, n_b, G)
    assert need > 0
    corr = torch.full((R, R), 7.0, device="cuda")
    stats = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((need // 4 + 8,), 7.0, device="cuda")
    big = torch.full(((1 << 20),), 7.0, device="cuda")  # (ample for every refused shape below)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    good = (n_a, n_b, G, p(a), G, p(b), G, p(corr), R, p(stats), p(ws), need, s)

    def call(**kw):
        names = ("n_a", "n_b", "G", "a", "lda", "b", "ldb", "corr", "ldc", "stats", "ws", "ws_bytes", "stream")
        args = dict(zip(names, good))
        args.update(kw)
        return lib.mmvae_stats_row_corr_f32(*[args[n] for n in names])

    refused = {
        "R < 2": dict(n_a=1, n_b=0, b=None, ldb=0),
        "R > 2048": dict(n_a=2000, n_b=49, ws=p(big), ws_bytes=big.numel() * 4),
        "G < 2": dict(G=1, ws=p(big), ws_bytes=big.numel() * 4),
        "n_a < 1": dict(n_a=0, n_b=4, ws=p(big), ws_bytes=big.numel() * 4),
        "n_b < 0": dict(n_b=-1, ws=p(big), ws_bytes=big.numel() * 4),
        "lda < G": dict(lda=G - 1),
        "ldb < G": dict(ldb=G - 1),
        "ldc < R": dict(ldc=R - 1),
        "null stats": dict(stats=None),
        "null a": dict(a=None),
        "null b with n_b > 0": dict(b=None),
        "b with n_b == 0": dict(n_b=0),
        "short workspace": dict(ws_bytes=need - 8),
        "no workspace": dict(ws=None),
        "misaligned workspace": dict(ws=p(ws, 4)),
    }
    for what, kw in refused.items():
        assert call(**kw) == _lib.ERR_ARG, what
    torch.cuda.synchronize()
    assert (corr == 7.0).all() and (stats == 7.0).all() and (ws == 7.0).all() and (big == 7.0).all()  # nothing ran
    assert call() == _lib.OK
    torch.cuda.synchronize()
    want, want_stats = ops.row_corrcoef(a, b)
    assert torch.equal(bits(corr), bits(want)) and torch.equal(bits(stats), bits(want_stats))
    assert call(corr=None, ldc=0) == _lib.OK  # corr is optional
    with pytest.raises(_lib.HipLibraryError, match="MMVAE_ERR_ARG"):
        ops.row_corrcoef(a[:1], None)
    with pytest.raises(ValueError):
        ops.row_corrcoef(a, b[:, :G - 1])
    torch.cuda.synchronize()


def test_graph_capture_and_replay(ops):
    case = CASES[3]
    a, b = make_inputs(*case)
    a2, b2 = make_inputs(*case[:5], seed=case[5] + 17)
    ta, tb = dev(a), dev(b)
    eager = [ops.row_corrcoef(dev(m), dev(n)) for m, n in ((a, b), (a2, b2))]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        corr, stats = ops.row_corrcoef(ta, tb)
    for (m, n), (want, want_stats) in zip(((a2, b2), (a, b)), (eager[1], eager[0])):
        ta.copy_(torch.from_numpy(m))
        tb.copy_(torch.from_numpy(n))
        corr.fill_(5.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(corr), bits(want)) and torch.equal(bits(stats), bits(want_stats))


def test_reference_shape(ops):
    """(100 + 100, 60 530): the reference's SAMPLE_SIZE cells per context by its human gene count, contiguous -- rows that
    are no 16-byte groups -- with log1p-normalised counts and a noisy, rectified copy as the cross generation."""
    from oracle.mmvae_oracle import synthetic_counts

    n, G = 100, 60530
    a = synthetic_counts(n, G).numpy().astype(np.float32)
    b = np.maximum(a + 0.25 * np.random.default_rng(2).standard_normal((n, G)), 0.0).astype(np.float32)
    a[3] = 0.0
    b[5] = np.float32(0.5)
    want = expected(a, b)
    assert want[2] == [1, 1]
    corr, stats = ops.row_corrcoef(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    check(corr, stats, want, "(100 + 100, 60530)")


def _trained_mirror(tmpdir, use_engine):
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    model = MU.build_mirror(case, "cuda", tmpdir, use_engine=use_engine)
    T = len(case["schedule"]) - 1
    MU.load_state(model, z, f"step{T}/sd/")
    model.eval()
    model.trainer.set_stage("validation")
    x, eps, _, _ = H.step_inputs(z, T)
    eid = str(z["eval/expert_id"])
    other = next(e for e in case["experts"] if e != eid)
    rng = np.random.default_rng(11)
    B = x.shape[0]
    x_other = np.maximum(rng.standard_normal((B, case["experts"][other])) - 0.4, 0.0).astype(np.float32)
    model.module.vae.encoder.explicit_eps = eps.cuda()
    batch_a = (x.cuda(), pd.DataFrame({"dummy": [0] * B}), eid)
    batch_b = (torch.from_numpy(x_other).cuda(), pd.DataFrame({"dummy": [1] * B}), other)
    return model, batch_a, batch_b, eid, other


def test_model_cross_species_correlation(tmp_path):
    model, batch_a, batch_b, eid, other = _trained_mirror(str(tmp_path / "engine"), True)
    keys = [f"{s}_{k}" for s in (eid, other) for k in ("cis", "cross", "comb", "rel")]
    model.validation_step(batch_a)
    model.predict_step(batch_a)
    engine = model._engine
    assert engine, "the captured engine must have taken this configuration"
    before = {k: id(p) for k, p in engine._plans.items() if k[0] != "generate"}
    assert {k[0] for k in before} == {"validate", "embed"}

    got = model.cross_species_correlation(batch_a, batch_b, decimals=None)
    rounded = model.cross_species_correlation(batch_a, batch_b)
    assert list(got) == keys and list(rounded) == keys
    assert engine.last_forward_key[0] == "generate"
    assert {k: id(p) for k, p in engine._plans.items() if k[0] != "generate"} == before  # other programs untouched

    out_a, out_b = model.cross_generate_step(batch_a), model.cross_generate_step(batch_b)
    by_hand, by_hand_rounded = {}, {}
    for s, cis, cross in ((eid, out_a, out_b), (other, out_b, out_a)):
        for store, decimals in ((by_hand, None), (by_hand_rounded, 3)):
            d = model.cell_correlation(cis[f"xhat_{s}"][0], cross[f"xhat_{s}"][0], decimals=decimals)
            store.update({f"{s}_{k}": d[k] for k in ("cis", "cross", "comb", "rel")})
    assert got == by_hand and rounded == by_hand_rounded

    twin, twin_a, twin_b, _, _ = _trained_mirror(str(tmp_path / "module"), False)
    module_path = twin.cross_species_correlation(twin_a, twin_b, decimals=None)
    assert not twin._engine and list(module_path) == keys
    for k in keys:
        print(f"{k}: engine {got[k]:.9f} module path {module_path[k]:.9f}")
        if k.endswith("_rel") and got[k[:-3] + "cis"] + got[k[:-3] + "cross"] < 0.1:
            continue
        assert abs(got[k] - module_path[k]) <= BOUND, (k, got[k], module_path[k])
