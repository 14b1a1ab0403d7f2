"""LayerNorm in ordinary FCBlocks (Linear -> [BatchNorm] -> LayerNorm(no affine) -> [ReLU] -> [Dropout]; the shared VAE's
encoder of the reference's configs/model/configV3.yaml), CPU side: the oracle and the mirror's module path against vectors
the reference's own modules produced (tests/golden/ln_core.npz, ln_mixed.npz; generator: tests/golden/make_golden_ln.py),
and the reasons the step engine gives for the models it declines.  Tolerances are those of tests/test_oracle_golden.py
and tests/mirror_utils.py for the small cases."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import mmvae_oracle as O
from tests import helpers as H
from tests import ln_cases as LC
from tests import mirror_utils as MU


@pytest.mark.parametrize("name", LC.LN_CASES)
def test_oracle_layernorm_steps_match_reference(name):
    case, z = H.load_case(name)
    spec = LC.spec_from_ln_case(case)
    hp = H.hparams_from_case(case)
    sd = H.sd_from(z, "sd0/")
    skip = H.bn_fed_biases(spec)
    assert any(spec.vae_encoder.use_layer_norm) and len(spec.adversarials) >= 1
    opt_state = {}
    for t, eid in enumerate(case["schedule"]):
        x, eps, masks, labels = H.step_inputs(z, t)
        out, sd_new = O.train_step(spec, sd, opt_state, x, eid, eps, masks, labels or None, case["kl_weights"][t], hp)
        g = lambda k: torch.from_numpy(np.array(z[f"step{t}/out/{k}"]))  # noqa: E731
        for k in ("loss", "recon_loss", "kl_loss", "Mean", "Variance", "total_loss"):
            torch.testing.assert_close(out[k], g(k), rtol=2e-6, atol=1e-6, msg=lambda m: f"{name} step{t} {k}: {m}")
        torch.testing.assert_close(out["z"], g("z"), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(out["xhat"], g("xhat"), rtol=1e-5, atol=1e-5)
        assert len(out["hidden"]) >= 2
        for i, h in enumerate(out["hidden"]):
            torch.testing.assert_close(h, g(f"hidden/{i}"), rtol=1e-5, atol=1e-5)
        for k, v in out["grad_norms"].items():
            torch.testing.assert_close(v, g(f"grad_norms/{k}"), rtol=1e-5, atol=1e-6, msg=lambda m: f"{k}: {m}")
        for phase in ("discriminator", "generator"):
            for i, a in enumerate(out.get(phase, []), start=1):
                torch.testing.assert_close(a["summed"], g(f"{phase}_{i}/summed"), rtol=1e-5, atol=1e-5)
                for cond, v in a["heads"].items():
                    torch.testing.assert_close(v, g(f"{phase}_{i}/{cond}"), rtol=1e-5, atol=1e-5)
        for n, gr in out["grads"].items():
            if n not in skip:
                assert H.rel_l2(gr, z[f"step{t}/grad/{n}"]) < 1e-4, f"{name} step{t} grad {n}"
        for n, v in sd_new.items():
            ref = z[f"step{t}/sd/{n}"]
            if n in skip:  # chaotic by construction (helpers.bn_fed_biases): bounded by the Adam step size
                assert np.abs(v.numpy() - ref).max() <= 2 * hp.lr * (t + 1) + 1e-6, n
            elif v.dtype == torch.int64:
                assert int(v) == int(ref), n
            elif n.endswith("running_mean") and t > 0:
                assert np.abs(v.detach().numpy() - ref).max() <= hp.bn_momentum * hp.lr * (t + 1) * (t + 2) + 1e-6, n
            else:
                assert H.rel_l2(v, ref) < 1e-4, f"{name} step{t} param {n}: {H.rel_l2(v, ref)}"
        sd = sd_new


@pytest.mark.parametrize("name", LC.LN_CASES)
def test_oracle_layernorm_eval_matches_reference(name):
    case, z = H.load_case(name)
    spec, hp = LC.spec_from_ln_case(case), H.hparams_from_case(case)
    T = len(case["schedule"]) - 1
    sd = H.sd_from(z, f"step{T}/sd/")
    x, eps, _, _ = H.step_inputs(z, T)
    eid = str(z["eval/expert_id"])
    out = O.eval_step(spec, sd, x, eid, eps, 1.0, hp)
    for k in ("loss", "recon_loss", "kl_loss"):
        torch.testing.assert_close(out[k], torch.from_numpy(np.array(z[f"eval/out/{k}"])), rtol=1e-4, atol=1e-5)
    assert H.rel_l2(out["z"], z["eval/out/z"]) < 1e-5
    assert H.rel_l2(out["xhat"], z["eval/out/xhat"]) < 1e-5
    assert H.rel_l2(O.latent_embeddings(spec, sd, x, eid, eps, hp), z["eval/out/embedding_z"]) < 1e-5


@pytest.mark.parametrize("name", LC.LN_CASES)
def test_mirror_layernorm_steps_on_cpu_plumbing_match_reference(name, monkeypatch):
    LC.patch(monkeypatch)
    case, z, results = MU.replay_training(name, "cpu")
    MU.check_against_golden(case, z, results)


def test_layernorm_state_dict_keys_match_reference():
    import tempfile

    from mmvae_amd import backend

    for name in LC.LN_CASES:
        case, z = H.load_case(name)
        with tempfile.TemporaryDirectory() as d, backend.cpu_plumbing():
            model = LC.build_ln_mirror(case, "cpu", d)
        assert set(model.module.state_dict().keys()) == {k[len("sd0/"):] for k in z.files if k.startswith("sd0/")}


def _model(tmpdir, **vae_kwargs):
    from mmvae_amd import backend
    from mmvae_amd.models import CMMVAEModel
    from mmvae_amd.modules import CLVAE, CMMVAE, base

    enc_act = vae_kwargs.pop("enc_act", nn.ReLU)
    cfg = lambda layers, act=nn.ReLU, **kw: base.FCBlockConfig(  # noqa: E731
        layers=list(layers), dropout_rate=0.0, use_batch_norm=False, use_layer_norm=False, activation_fn=act, **kw)
    base.Adversarial.labels.clear()
    with backend.cpu_plumbing():
        vae = CLVAE(latent_dim=4, encoder_config=cfg([8, 6], act=enc_act), decoder_config=cfg([4, 6, 8]), **vae_kwargs)
        experts = base.Experts([base.Expert("human", cfg([16, 8]), cfg([8, 16]))])
        return CMMVAEModel(CMMVAE(vae, experts, None))


def test_decline_reason_names_the_cause(tmp_path):
    """The model-shape reasons come before the optimiser check, so they read the same on a host without a GPU."""
    from mmvae_amd.engine import StepEngine

    why = StepEngine.decline_reason(_model(str(tmp_path), distribution="ln"))
    assert why is not None and "distribution" in why and "ln" in why
    why = StepEngine.decline_reason(_model(str(tmp_path), enc_act=nn.Sigmoid))
    assert why is not None and "Sigmoid" in why and "activation" in why
    assert StepEngine.try_build(_model(str(tmp_path), enc_act=nn.Sigmoid)) is None


def test_decline_reason_takes_layernorm_blocks_by_shape(tmp_path):
    """LayerNorm in the shared VAE's blocks is no reason any more; in an adversary's encoder or on an expert decoder's
    last layer it is, by name.  (On this host the remaining reason for ln_core is the optimiser: no HIP Adam here.)"""
    import tempfile

    from mmvae_amd import backend
    from mmvae_amd.engine import StepEngine
    from mmvae_amd.engine_common import _block_decline
    from mmvae_amd.modules import base

    case, _ = H.load_case("ln_core")
    with tempfile.TemporaryDirectory() as d, backend.cpu_plumbing():
        model = LC.build_ln_mirror(case, "cpu", d)
        m = model.module
        assert hasattr(m.vae.encoder.fc.fc_layers[0], "ln")
        for b in (m.vae.encoder.fc, m.vae.decoder, m.experts["human"].encoder, m.experts["human"].decoder):
            assert _block_decline(b) is None
        why = StepEngine.decline_reason(model)
        assert why is None or "optimiser" in why
        ln_block = base.FCBlock(base.FCBlockConfig(layers=[24, 16, 8], dropout_rate=0.0, use_batch_norm=False,
                                                   use_layer_norm=True, activation_fn=nn.ReLU))
        m.adversarials[0].encoder = ln_block
        why = StepEngine.decline_reason(model)
        assert "adversary 1" in why and "LayerNorm" in why


@pytest.mark.parametrize("where,bn", [("encoder_first", False), ("encoder_first", True), ("decoder_last", False)])
def test_decline_reason_names_the_gene_wide_layernorm_placements(where, bn):
    """LayerNorm on an expert encoder's first layer (with or without BatchNorm) and on an expert decoder's last layer are
    the two placements in the experts that stay on the module path, each with its own reason."""
    import tempfile

    from mmvae_amd import backend
    from mmvae_amd.engine import StepEngine

    case, _ = H.load_case("ln_core")
    case = dict(case, blocks={k: dict(v) for k, v in case["blocks"].items()})
    if where == "encoder_first":
        case["blocks"]["expert_enc"].update(ln=[True, False], bn=[bn, True])
    else:
        case["blocks"]["expert_dec"].update(ln=[False, True])
    with tempfile.TemporaryDirectory() as d, backend.cpu_plumbing():
        model = LC.build_ln_mirror(case, "cpu", d)
        why = StepEngine.decline_reason(model)
        said = []
        assert StepEngine.try_build(model, on_decline=said.append) is None and said == [why]
    assert "LayerNorm" in why and "expert 'human'" in why
    assert ("first" in why and "encoder" in why) if where == "encoder_first" else ("last" in why and "decoder" in why)
