"""Host-side checks of the cross-generation feature (no GPU): the C-ABI surface of the per-gene correlation, the
"generate" layout, the module path of CMMVAEModel.cross_generate_step on CPU plumbing."""
import os
import re

import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(header: str, name: str) -> str:
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/mmvae_hip.h"
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_and_lib_binds_the_correlation_entry_points():
    from mmvae_amd import _lib

    header = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    lib = _lib.load()  # loads on a GPU-less host too (no compute call is made)
    for name in ("mmvae_col_pearson_f32", "mmvae_col_pearson_workspace_bytes"):
        n_args = len([a for a in _declaration(header, name).split(",") if a.strip() and a.strip() != "void"])
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name)
    assert len(_lib.PROTOTYPES["mmvae_col_pearson_f32"][1]) == 10
    # pure host helper: chunked fp64 partials, five moments per column; nothing for shapes the launch refuses
    assert lib.mmvae_col_pearson_workspace_bytes(1, 100) == 0 and lib.mmvae_col_pearson_workspace_bytes(100, 0) == 0
    for B, G in ((2, 5), (100, 60530), (512, 20000), (1024, 60530)):
        nbytes = lib.mmvae_col_pearson_workspace_bytes(B, G)
        assert nbytes % (5 * 8 * G) == 0 and 1 <= nbytes // (5 * 8 * G) <= (B + 31) // 32
    B, G = 3_000_000, 4  # millions of rows: the chunks grow so that their count stays inside the grid's y extent
    assert 1 <= lib.mmvae_col_pearson_workspace_bytes(B, G) // (5 * 8 * G) <= 65535
    # the shapes the kernel is meant for fill the chip: at least two workgroups of 256 columns per CU
    for B, G in ((100, 60530), (512, 20000), (1024, 60530)):
        chunks = lib.mmvae_col_pearson_workspace_bytes(B, G) // (5 * 8 * G)
        assert chunks * ((G + 255) // 256) >= 512


def test_abi_version_is_16():
    """15 added the per-gene correlation entries; 16 folded the reconstruction / FC-epilogue entry-point ladders."""
    from mmvae_amd import _lib

    header = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    assert int(re.search(r"#define\s+MMVAE_ABI_VERSION\s+(\d+)", header).group(1)) == 16
    assert _lib.load().mmvae_abi_version() == 16


def test_generate_layout_stays_on_one_stream():
    """plan_layout(mode="generate") at C2's geometry (B = 512, 20 000 genes, 1 024-wide last hidden layer) with every
    branch stream available: nothing is placed on a branch (forks are validated for the training geometry only)."""
    from mmvae_amd.engine import EngineSettings, plan_layout

    common = dict(fork_ok=True, side_stream=True, side_stream2=True, lane_stream=True, overlap=False, world=1, B=512, K=1,
                  R=512, G=20000, n_in_last=1024, iwae=False, has_adv=False, has_cond=False, adv_reducer=False)
    st = EngineSettings()
    train = plan_layout(st, mode="train", **common)
    assert train.side_dw and train.late and train.prefetch  # (the geometry the training forks are measured on)
    for has_adv in (False, True):
        L = plan_layout(st, mode="generate", **dict(common, has_adv=has_adv))
        assert not (L.side_dw or L.early or L.late or L.adv_aside or L.adv_dw2 or L.adv_lane or L.dp_dw or L.prefetch
                    or L.prefetch_side2)


def test_cross_generate_step_module_path_on_cpu_plumbing(tmp_path):
    from mmvae_amd import backend
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    with backend.cpu_plumbing():
        model = MU.build_mirror(case, "cpu", str(tmp_path), use_engine=True)
        T = len(case["schedule"]) - 1
        MU.load_state(model, z, f"step{T}/sd/")
        model.eval()
        x, eps, _, _ = H.step_inputs(z, T)
        eid = str(z["eval/expert_id"])
        metadata = pd.DataFrame({"dummy": [0] * x.shape[0]})
        model.module.vae.encoder.explicit_eps = eps
        out = model.cross_generate_step((x, metadata, eid))
        with torch.no_grad():
            _, _, zz, xhats, _ = model.module(x, metadata, eid, cross_generate=True)
        assert model._engine is None  # CPU tensors never reach the engine
        assert list(out) == ["z"] + [f"xhat_{e}" for e in case["experts"]]
        assert torch.equal(out["z"][0], zz) and out["z"][1] is metadata and (metadata["species"] == eid).all()
        for e in case["experts"]:
            assert torch.equal(out[f"xhat_{e}"][0], xhats[e])
            assert H.rel_l2(out[f"xhat_{e}"][0], z[f"eval/out/xhat_cross/{e}"]) < 2e-5
        one = model.cross_generate_step((x, metadata, eid), targets="mouse")
        assert list(one) == ["z", "xhat_mouse"] and torch.equal(one["xhat_mouse"][0], xhats["mouse"])
        try:
            model.cross_generate_step((x, metadata, eid), targets=["rat"])
            raise AssertionError("an unknown target must raise KeyError")
        except KeyError:
            pass
        r, mean_r, n_valid = model.gene_correlation(out["xhat_human"][0], out["xhat_human"][0])
        live = ~torch.isnan(r)
        assert int(n_valid) == int(live.sum()) and (r[live] == 1.0).all()


def test_nothing_under_the_package_imports_the_oracle():
    for dp, _, files in os.walk(os.path.join(ROOT, "mmvae_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"
