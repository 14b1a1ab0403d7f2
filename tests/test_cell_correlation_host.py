"""Host-side checks of the cell-by-cell correlation (no GPU): the C-ABI surface of libmmvae_stats.so, the workspace
helper, the fp64 CPU-plumbing statement against numpy and against the reference's own calc_correlations numbers
(tests/golden/cell_correlation.npz), and Trainer.correlations on the module path."""
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_stats.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cell_correlation.npz")
GOLDEN_CASES = ("split_7_5x70", "split_6_6x61")


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _stats_lib

    declared = check_surface(_stats_lib.BINDING)
    assert set(declared) == {"mmvae_stats_abi_version", "mmvae_stats_build_arch", "mmvae_stats_row_corr_workspace_bytes",
                             "mmvae_stats_row_corr_f32"} == set(_stats_lib.STATS_PROTOTYPES)
    assert declared["mmvae_stats_row_corr_f32"] == 13


def test_versions_and_arch():
    from mmvae_amd import _lib, _stats_lib

    header = open(HEADER).read()
    assert int(re.search(r"#define\s+MMVAE_STATS_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    lib = _stats_lib.load_stats()
    assert lib.mmvae_stats_abi_version() == 1 == _stats_lib.STATS_ABI_VERSION
    assert lib.mmvae_stats_build_arch() == b"gfx950"
    # the training library is untouched: same version, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_stats_")]
    assert not hasattr(_lib.load(), "mmvae_stats_row_corr_f32")


def test_workspace_helper():
    from mmvae_amd import _stats_lib

    need = _stats_lib.load_stats().mmvae_stats_row_corr_workspace_bytes
    for n_a, n_b, G in ((1, 0, 70), (2049, 0, 70), (1024, 1025, 70), (2, 2, 1), (0, 4, 70), (-1, 4, 70), (4, -1, 70)):
        assert need(n_a, n_b, G) == 0, (n_a, n_b, G)
    for n_a, n_b, G in ((1, 1, 2), (100, 100, 60530), (512, 512, 20000), (2048, 0, 70)):
        nbytes = need(n_a, n_b, G)
        assert nbytes > 0 and nbytes % 8 == 0, (n_a, n_b, G, nbytes)
    # depends on the stacked row count only: the same rows divided differently need the same workspace
    assert need(100, 100, 20000) == need(200, 0, 20000) == need(37, 163, 20000)


def _relu_like(rng, n, G, shared, shift=0.4):
    return np.maximum(rng.standard_normal((n, G)) + 0.8 * shared - shift, 0.0).astype(np.float32)


def test_cpu_plumbing_statement_matches_numpy():
    from mmvae_amd import backend
    from mmvae_amd import functional as HF

    rng = np.random.default_rng(5)
    G = 131
    shared = rng.standard_normal(G)
    a, b = _relu_like(rng, 9, G, shared), _relu_like(rng, 6, G, shared)
    a[2] = 0.0
    b[4] = 2.5
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.corrcoef(np.vstack([a, b]).astype(np.float64))
    with backend.cpu_plumbing():
        corr, stats = HF.row_corrcoef(torch.from_numpy(a), torch.from_numpy(b))
        stacked, stats_stacked = HF.row_corrcoef(torch.from_numpy(np.vstack([a, b])))
        none, stats_only = HF.row_corrcoef(torch.from_numpy(a), torch.from_numpy(b), want_matrix=False)
    got = corr.numpy()
    assert corr.dtype == torch.float64 and stats.dtype == torch.float64 and stats.shape == (8,)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[2]).all() and np.isnan(got[:, 9 + 4]).all()
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-12
    assert torch.equal(torch.nan_to_num(stacked), torch.nan_to_num(corr)) and none is None
    assert torch.equal(stats_only, stats)
    z = np.nan_to_num(want)
    cis, cross, comb = z[:9, :9].mean(), z[9:, 9:].mean(), z[:9, 9:].mean()
    assert np.allclose(stats.numpy()[:4], [cis, cross, comb, 2 * comb / (cis + cross)], rtol=0, atol=1e-12)
    assert stats.numpy()[4:].tolist() == [1.0, 1.0, 0.0, 0.0]
    s = stats_stacked.numpy()  # no second operand: numpy's mean over nothing
    assert abs(s[0] - z.mean()) <= 1e-12 and np.isnan(s[1:4]).all() and s[4:].tolist() == [2.0, 0.0, 0.0, 0.0]


def test_cpu_tensor_is_refused_outside_cpu_plumbing():
    from mmvae_amd import functional as HF
    from mmvae_amd import ops
    from mmvae_amd._lib import HipLibraryError
    from mmvae_amd.models.cmmvae_model import CMMVAEModel

    a = torch.rand(4, 10)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        HF.row_corrcoef(a, a)
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        CMMVAEModel.cell_correlation(a, a)
    with pytest.raises(HipLibraryError):
        ops.row_corrcoef(a, a)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_cell_correlation_reproduces_the_reference_numbers(name):
    """The eight numbers calc_correlations itself returned for these inputs (make_cell_correlation_golden.py), exactly."""
    from mmvae_amd import backend
    from mmvae_amd.models.cmmvae_model import CMMVAEModel

    z = np.load(GOLDEN)
    n = int(z[f"{name}/n"])
    got, unrounded = [], []
    with backend.cpu_plumbing():
        for species in ("human", "mouse"):
            x = torch.from_numpy(z[f"{name}/{species}"])
            d = CMMVAEModel.cell_correlation(x[:n], x[n:], decimals=3)
            assert list(d) == ["cis", "cross", "comb", "rel", "n_constant"] and d["n_constant"] == 1
            got += [d[k] for k in ("cis", "cross", "comb", "rel")]
            u = CMMVAEModel.cell_correlation(x[:n], x[n:], decimals=None)
            unrounded.append(u)
            with np.errstate(divide="ignore", invalid="ignore"):
                c = np.nan_to_num(np.corrcoef(z[f"{name}/{species}"].astype(np.float64)))
            want = [c[:n, :n].mean(), c[n:, n:].mean(), c[:n, n:].mean()]
            assert np.allclose([u["cis"], u["cross"], u["comb"]], want, rtol=0, atol=1e-12)
            assert abs(u["rel"] - 2 * want[2] / (want[0] + want[1])) <= 1e-12
            assert [np.round(u[k], 3) for k in ("cis", "cross", "comb")] == [d[k] for k in ("cis", "cross", "comb")]
            assert u["cis"] != d["cis"]  # (really unrounded)
    assert got == z[f"{name}/expected"].tolist()


def _two_groups(case, z):
    """Two (group_id, batch_a, batch_b) groups over the golden inputs of a two-expert case, group ids out of order."""
    from tests import helpers as H

    T = len(case["schedule"]) - 1
    x, eps, _, _ = H.step_inputs(z, T)
    eid = str(z["eval/expert_id"])
    other = next(e for e in case["experts"] if e != eid)
    rng = np.random.default_rng(11)
    B = x.shape[0]
    groups = []
    for gid in (7, 3):
        xa = x if gid == 7 else torch.from_numpy(_relu_like(rng, B, case["experts"][eid], 0.0))
        xb = torch.from_numpy(_relu_like(rng, B, case["experts"][other], 0.0))
        md_a = pd.DataFrame({"sex": [f"sex_{gid}"] * B, "tissue": ["lung"] + ["liver"] * (B - 1), "dummy": [0] * B})
        md_b = pd.DataFrame({"dummy": [1] * B})
        groups.append((gid, (xa, md_a, eid), (xb, md_b, other)))
    return groups, eps, eid, other


def test_trainer_correlations_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend
    from mmvae_amd.trainer import Trainer
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    with backend.cpu_plumbing():
        model = MU.build_mirror(case, "cpu", str(tmp_path), use_engine=True)
        MU.load_state(model, z, f"step{len(case['schedule']) - 1}/sd/")
        groups, eps, eid, other = _two_groups(case, z)
        model.module.vae.encoder.explicit_eps = eps
        table = Trainer().correlations(model, groups)
        assert not model.module.training
        stat_cols = [f"{s}_{k}" for s in (eid, other) for k in ("cis", "cross", "comb", "rel")]
        assert list(table.columns) == ["group_id", "num_samples"] + stat_cols + ["sex", "tissue"]
        assert table["group_id"].tolist() == [3, 7] and table["num_samples"].tolist() == [groups[0][1][0].shape[0]] * 2
        assert table["sex"].tolist() == ["sex_3", "sex_7"] and table["tissue"].tolist() == ["lung", "lung"]
        for gid, batch_a, batch_b in groups:  # by hand: two cross_generate_step calls, cell_correlation per expert
            out_a, out_b = model.cross_generate_step(batch_a), model.cross_generate_step(batch_b)
            want = {}
            for s, cis, cross in ((eid, out_a, out_b), (other, out_b, out_a)):
                d = model.cell_correlation(cis[f"xhat_{s}"][0], cross[f"xhat_{s}"][0])
                want.update({f"{s}_{k}": d[k] for k in ("cis", "cross", "comb", "rel")})
            row = table[table["group_id"] == gid].iloc[0]
            assert [row[c] for c in stat_cols] == [want[c] for c in stat_cols], gid
            assert model.cross_species_correlation(batch_a, batch_b) == want
            unrounded = model.cross_species_correlation(batch_a, batch_b, decimals=None)
            assert list(unrounded) == stat_cols
            assert all(abs(unrounded[c] - want[c]) <= 5.0001e-4 for c in stat_cols if not c.endswith("_rel"))
        with pytest.raises(ValueError):
            model.cross_species_correlation(groups[0][1], groups[0][1])
