"""LayerNorm FCBlock layers on the GPU: the fused row tail (mmvae_fc_rowtail_fwd / _bwd) against fp64 autograd, and the
captured step engine on models that have such layers -- against the reference's vectors (tests/golden/ln_core.npz,
ln_mixed.npz), against the oracle through the replayed program with device noise (oracle/program_check.py), in the
validation / predict programs and with K = 5 samples.  Tolerances are the neighbouring tests' (stated at each test)."""
import tempfile
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import ln_cases as LC  # noqa: E402
from tests import mirror_utils as MU  # noqa: E402

DECLINED = "captured step engine does not cover"


# ------------------------------------------------------------------------------------------------------ kernel
def _rowtail_reference(slabs, bias, eps, slope, mask, p, gout, addend, row_scale):
    """fp64 autograd of the tail: (y, a, d, dz, dbias).  `slope`: the 0/1 ReLU slope the kernel took (None: no ReLU) --
    an input within rounding of zero may fall on either side in fp32; its value is below the tolerance either way."""
    v = (slabs.double().sum(0) + (bias.double() if bias is not None else 0.0)).requires_grad_(True)
    y = torch.nn.functional.layer_norm(v, (v.shape[1],), eps=eps)
    a = y * slope.double() if slope is not None else y
    d = a * mask.double() / (1.0 - p) if mask is not None else a
    g = gout.double().sum(0)
    if row_scale is not None:
        g = g * row_scale.double()[:, None]
    loss = (d * g).sum() + ((a * addend.double()).sum() if addend is not None else 0.0)
    (dz,) = torch.autograd.grad(loss, v)
    return y.detach(), a.detach(), d.detach(), dz, dz.sum(0)


@pytest.mark.parametrize("rows,N,S,S_in,relu,p,use_addend,use_scale,use_bias", [
    (512, 768, 1, 1, True, 0.0, False, False, True),     # configV3's first VAE layer
    (512, 768, 4, 3, True, 0.1, True, False, True),      # several slabs both ways, mask, hidden gradient
    (37, 33, 2, 1, False, 0.0, False, True, True),       # rows off the 32-row chunk, odd N, no activation, row weights
    (100, 257, 1, 2, True, 0.25, True, True, False),     # odd N just over a register class, no bias (behind a BatchNorm)
    (64, 512, 3, 1, False, 0.2, False, False, True),     # dropout without ReLU
    (33, 1024, 1, 1, True, 0.0, True, False, True),      # the widest register-resident row
    (70, 1100, 2, 2, True, 0.1, True, True, True),       # beyond it: the looping kernels + the column pass
])
def test_rowtail_kernel_matches_fp64_autograd(rows, N, S, S_in, relu, p, use_addend, use_scale, use_bias):
    """Outputs rtol = atol = 1e-5, dz and the bias gradient rel-L2 < 2e-5 (the bounds of the column kernels' tests in
    tests/test_kernels_gpu.py); two runs give bit-identical bias gradients."""
    from mmvae_amd import ops

    g = torch.Generator().manual_seed(rows * 1000 + N)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    slabs, bias = r(S, rows, N), (0.3 * r(N) if use_bias else None)
    mask = (torch.rand(rows, N, generator=g) >= p).to(torch.uint8) if p > 0 else None
    gout = r(S_in, rows, N)
    addend = r(rows, N) if use_addend else None
    row_scale = torch.rand(rows, generator=g) + 0.5 if use_scale else None
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    out = ops.fc_rowtail_fwd(dev(slabs), dev(bias), eps=1e-5, relu=relu, keep_mask=dev(mask), dropout_p=p)
    runs = [ops.fc_rowtail_bwd(dev(gout), out["y"], out["invstd"], addend=dev(addend), row_scale=dev(row_scale),
                               keep_mask=dev(mask), dropout_p=p, relu=relu, act=out["a"]) for _ in range(2)]
    torch.cuda.synchronize()
    slope = (out["a"] > 0).cpu() if relu else None
    y, a, d, dz, dbias = _rowtail_reference(slabs, bias, 1e-5, slope, mask, p, gout, addend, row_scale)
    if relu:  # the slope the kernel took may differ from 1[y > 0] of the fp64 rows only at a kink: |y| <= 1e-4 rms(y),
        kinks = slope != (y > 0)  # the rule of mirror_utils.compare_with_oracle_at_given_slopes
        rms = float(y.pow(2).mean().sqrt())
        assert not kinks.any() or float(y[kinks].abs().max()) <= 1e-4 * rms, (int(kinks.sum()), float(y[kinks].abs().max()))
    for name, got, want in (("y", out["y"], y), ("a", out["a"], a), ("d", out["d"], d)):
        err = float((got.cpu().double() - want).abs().max())
        print(f"rowtail fwd {rows}x{N} {name}: max abs error {err:.3e}")
        torch.testing.assert_close(got.cpu().double(), want, rtol=1e-5, atol=1e-5, msg=lambda m: f"{name}: {m}")
    var = (slabs.double().sum(0) + (bias.double() if bias is not None else 0.0)).var(1, unbiased=False)
    torch.testing.assert_close(out["invstd"].cpu().double(), 1.0 / torch.sqrt(var + 1e-5), rtol=1e-5, atol=1e-5)
    e_dz, e_db = H.rel_l2(runs[0][0], dz), H.rel_l2(runs[0][1], dbias)
    print(f"rowtail bwd {rows}x{N}: dz rel-L2 {e_dz:.3e}, dbias rel-L2 {e_db:.3e}")
    assert e_dz < 2e-5 and e_db < 2e-5
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])
    # eval mode: the same output without a mask, nothing saved
    ev = ops.fc_rowtail_fwd(dev(slabs), dev(bias), eps=1e-5, training=False, relu=relu)
    assert ev["invstd"] is None
    torch.testing.assert_close(ev["d"].cpu().double(), a, rtol=1e-5, atol=1e-5)


def test_rowtail_rejects_bad_arguments():
    from mmvae_amd import _lib

    lib = _lib.load()
    x = torch.zeros(8, 16, device="cuda")
    m = torch.ones(8, 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731
    # a keep mask in eval mode; training without a place for invstd; a leading dimension below N; no workspace for dbias
    assert lib.mmvae_fc_rowtail_fwd(8, 16, P(x), 16, 1, None, 1e-5, 0, 0, P(m), 0.1, None, None, P(x), 16, None, s) == _lib.ERR_ARG
    assert lib.mmvae_fc_rowtail_fwd(8, 16, P(x), 16, 1, None, 1e-5, 1, 0, None, 0.0, None, None, P(x), 16, None, s) == _lib.ERR_ARG
    assert lib.mmvae_fc_rowtail_fwd(8, 16, P(x), 8, 1, None, 1e-5, 0, 0, None, 0.0, None, None, P(x), 16, None, s) == _lib.ERR_ARG
    assert lib.mmvae_fc_rowtail_bwd(8, 16, P(x), 16, 1, None, None, None, 0.0, 0, None, P(x), P(x), P(x), 16, P(x), None, 0,
                                    s) == _lib.ERR_WORKSPACE
    assert lib.mmvae_fc_rowtail_bwd(8, 16, P(x), 16, 1, None, None, None, 0.0, 0, None, P(x), P(x), P(x), 16, None, P(x), 8,
                                    s) == _lib.ERR_WORKSPACE


# ---------------------------------------------------------------------------------------- engine against the reference
@pytest.mark.parametrize("name", LC.LN_CASES)
def test_module_path_matches_reference_with_layernorm(name, monkeypatch):
    LC.patch(monkeypatch)
    case, z, results = MU.replay_training(name, "cuda", use_engine=False)
    MU.check_against_golden(case, z, results)


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("name", LC.LN_CASES)
def test_engine_takes_layernorm_models_and_matches_reference(name, overlap, monkeypatch):
    """The bounds of tests/test_step_gpu.py::test_engine_path_matches_reference (mirror_utils.check_against_golden: losses
    rtol 2e-5, gradient norms 5e-5, post-step parameters and BatchNorm buffers rel-L2 1e-4 over three steps, so the Adam
    moments of the earlier steps are in the later ones).  overlap: the data-parallel exchange program forced on one rank."""
    from mmvae_amd.engine import StepEngine

    if overlap:
        monkeypatch.setenv("MMVAE_DP_OVERLAP", "1")
    LC.patch(monkeypatch)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        case, z, results = MU.replay_training(name, "cuda", use_engine=True)
    engine = MU.replay_training.last_engine
    assert isinstance(engine, StepEngine), "the captured engine must take LayerNorm FCBlocks"
    assert not [w for w in seen if DECLINED in str(w.message)]
    MU.check_against_golden(case, z, results)
    plans = [p for k, p in engine._plans.items() if str(k[0]).startswith("train")]
    assert plans and all(any(l.ln is not None for l in p.enc_layers + p.dec_layers) for p in plans)
    for p in plans:  # the row tail's saved rows exist where the backward pass needs them apart from .d
        for l in p.enc_layers + p.dec_layers:
            if l.ln is not None:
                assert l.ln_invstd is not None and (l.y is not None) == (l.relu or l.p > 0)


@pytest.mark.parametrize("use_engine", [False, True])
@pytest.mark.parametrize("name", LC.LN_CASES)
def test_layernorm_eval_and_predict_programs_match_reference(name, use_engine, tmp_path):
    """validation_step / predict_step on the reference's post-training state: losses rtol 1e-4, tensors rel-L2 2e-5 (the
    bounds of tests/test_step_gpu.py::test_eval_and_predict_paths_match_reference); engine and module path on the same
    weights then agree with each other to twice that."""
    from mmvae_amd.engine import StepEngine

    case, z = H.load_case(name)
    T = len(case["schedule"]) - 1
    x, eps, _, labels = H.step_inputs(z, T)
    eid = str(z["eval/expert_id"])
    metadata = pd.DataFrame({cond: [f"{cond}_{int(i)}" for i in idx] for cond, idx in labels.items()})
    model = LC.build_ln_mirror(case, "cuda", str(tmp_path), use_engine=use_engine)
    MU.load_state(model, z, f"step{T}/sd/")
    model.eval()
    model.trainer.set_stage("validation")
    model.module.vae.encoder.explicit_eps = eps.cuda()
    with torch.no_grad():
        ld = model.validation_step((x.cuda(), metadata, eid))
        emb = model.predict_step((x.cuda(), metadata, eid))
        torch.cuda.synchronize()
    for k in ("loss", "recon_loss", "kl_loss"):
        ref = float(np.array(z[f"eval/out/{k}"]))
        assert abs(float(ld[k]) - ref) <= 1e-4 * abs(ref) + 1e-5, (k, float(ld[k]), ref)
    assert H.rel_l2(emb["z"][0], z["eval/out/embedding_z"]) < 2e-5
    if use_engine:
        assert isinstance(model._engine, StepEngine)
        assert {k[0] for k in model._engine._plans} == {"validate", "embed"}
        model._engine.close()


def test_layernorm_k5_step_matches_oracle(tmp_path, monkeypatch):
    """K = 5 samples through the engine on the ln_core model (with its adversary): the K > 1 route of
    tests/test_configs_gpu.py -- the oracle on the host with the same eps [K, B, Z] and masks at the engine's ReLU slopes;
    losses and gradient norms 1e-4, gradients as full tensors 5e-4, parameters of the cold step 1e-3."""
    from mmvae_amd.engine import StepEngine
    from oracle import mmvae_oracle as O  # noqa: F401

    LC.patch(monkeypatch)
    K = 5
    case, z = H.load_case("ln_core")
    eid = case["schedule"][0]
    x, _, masks, labels = H.step_inputs(z, 0)
    eps = torch.randn(K, x.shape[0], case["Z"], generator=torch.Generator().manual_seed(5))
    model = LC.build_ln_mirror(case, "cuda", str(tmp_path), use_engine=True)
    MU.load_state(model, z, "sd0/")
    sd_in = {k: v.detach().cpu().clone() for k, v in model.module.state_dict().items()}
    model.train()
    model.trainer.set_stage("training")
    model.module.vae.encoder.n_samples = K
    model.kl_annealing_fn.kl_weight = 1.0
    model.module.vae.encoder.explicit_eps = eps.cuda()
    MU.set_explicit_masks(model, masks, eid, "cuda")
    metadata = pd.DataFrame({cond: [f"{cond}_{int(i)}" for i in idx] for cond, idx in labels.items()})
    model.logged.clear()
    model.training_step((x.cuda(), metadata, eid), 0)
    model._flush_engine()
    torch.cuda.synchronize()
    assert isinstance(model._engine, StepEngine) and model._engine.last_plan.K == K
    names = {id(p): n for n, p in model.module.named_parameters()}
    grads = {}
    for o in model.optimizers():
        for i, p in enumerate(o.arena.params):
            if names[id(p)].startswith(("vae.", f"experts.{eid}.")):
                grads[names[id(p)]] = o.arena.grad_view(i).detach().cpu().clone()
    sd = {k: v.detach().cpu().clone() for k, v in model.module.state_dict().items()
          if k.startswith(("vae.", f"experts.{eid}.", "adversarials."))}
    logged = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in model.logged.items()}
    kinks, wg, wp, ref = MU.compare_with_oracle_at_given_slopes(model, case, eid, sd_in, 0, {}, x, eps, masks, labels, 1.0,
                                                                 sd, grads, tol=5e-4)
    print(f"K = 5: {kinks} kinks, worst gradient rel-L2 {wg:.3e}, worst parameter rel-L2 {wp:.3e}")
    for k, v in (("loss", ref["total_loss"]), ("recon_loss", ref["recon_loss"]), ("kl_loss", ref["kl_loss"])):
        assert abs(logged[f"{k}/training/{eid}"] - float(v)) <= 1e-4 * abs(float(v)), (k, logged[f"{k}/training/{eid}"], float(v))
    for key, name in (("vae", "grad_norms/vae"), (f"expert_{eid}", f"grad_norms/expert_{eid}")):
        want = float(ref["grad_norms"][key])
        assert abs(logged[name] - want) <= 1e-4 * want, (name, logged[name], want)
    model._engine.close()


# ---------------------------------------------------------------------------- the replayed program against the oracle
def test_layernorm_core_replayed_program_matches_oracle():
    """configV3's core widths (shared VAE encoder [768, 512, 256, 256] with LayerNorm + ReLU, Z = 128), two experts of a few
    thousand genes, B = 512: every step is taken the way a training loop takes it -- resident batches, Philox noise, the
    captured graph from a plan's second run on -- and held to oracle.program_check's own TOL (strict), cold and warm."""
    from mmvae_amd import synthetic
    from mmvae_amd.engine import StepEngine
    from oracle import program_check as PC

    experts = {"human": 3000, "mouse": 2504}
    B = 512
    model = synthetic.build_layernorm_core_model(experts, use_engine=True, seed=3).to("cuda")
    model.train()
    model.trainer.set_stage("training")
    model.optimizers()
    data = {eid: (synthetic.synthetic_counts(B, G, seed=77 + i, device="cuda"), synthetic.synthetic_metadata(B, seed=5))
            for i, (eid, G) in enumerate(experts.items())}
    eids = list(experts)
    rows = []
    for step in range(8):
        eid = eids[step % 2]
        x, meta = data[eid]
        r = PC.check_step(model, eid, x, meta, step, strict=True)
        plan = model._engine.last_plan
        print(f"step {step} ({eid}): run {plan._runs} of its plan, {r}")
        assert isinstance(model._engine, StepEngine) and r["philox"]
        assert r["replayed"] == (plan._runs >= 2), (step, plan._runs, r["replayed"])
        assert not r["forked"]  # (a few thousand genes: outside the geometry at which plans fork side branches)
        rows.append(r)
    assert rows[0]["cold"] and rows[1]["cold"] and not rows[-1]["cold"]
    assert sum(1 for r in rows if r["replayed"]) >= 4
    plan = model._engine.last_plan
    ln_layers = [l for l in plan.enc_layers if l.ln is not None]
    assert [l.n_out for l in ln_layers] == [512, 256, 256]
    model._engine.close()


# --------------------------------------------------------------------------------------------- no silent fallback
def test_one_warning_with_the_reason_for_a_declined_model():
    """The model path says once per model why the engine declined; a model the engine takes says nothing (checked in
    test_engine_takes_layernorm_models_and_matches_reference)."""
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        MU.replay_training("ln_dist", "cuda", use_engine=True)  # three training steps on one model
    assert not MU.replay_training.last_engine
    mine = [str(w.message) for w in seen if DECLINED in str(w.message)]
    assert len(mine) == 1 and "distribution" in mine[0], mine
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        MU.replay_training("ln_dist", "cuda", use_engine=False)
    assert not [w for w in seen if DECLINED in str(w.message)]
