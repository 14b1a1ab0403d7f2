"""Learning-rate schedules and the AdamW choice on the model surface, without a GPU: schedule values, a model node in
the LightningCLI YAML schema with `lr_schedule_fn:` / `optim_cls:`, the learning rate every optimiser has at each
training step of a golden case, and HipAdam's decoupled rule (CPU plumbing) against torch.optim.AdamW."""
import math

import pytest
import torch
import yaml

from tests import helpers as H
from tests import mirror_utils as MU


def test_warmup_cosine_values():
    from mmvae_amd.modules.base import LRScheduleFn, WarmupCosineLRFn

    assert [LRScheduleFn().factor(t) for t in (0, 7, 10 ** 6)] == [1.0, 1.0, 1.0]
    warmup, total, low = 10, 50, 0.1
    fn = WarmupCosineLRFn(warmup, total, min_factor=low)
    cos_at = lambda t: low + (1 - low) * 0.5 * (1 + math.cos(math.pi * (t - warmup) / (total - warmup)))  # noqa: E731
    assert fn.factor(0) == pytest.approx(1 / warmup, rel=1e-12)
    assert fn.factor(warmup - 1) == pytest.approx(1.0, rel=1e-12)
    assert fn.factor(warmup) == pytest.approx(1.0, rel=1e-12)  # the cosine starts at its top
    mid = (warmup + total) // 2
    assert fn.factor(mid) == pytest.approx((1 + low) / 2, rel=1e-12)  # half-way down the cosine
    assert fn.factor(mid) == pytest.approx(cos_at(mid), rel=1e-12)
    assert fn.factor(total - 1) == pytest.approx(cos_at(total - 1), rel=1e-12)
    assert low < fn.factor(total - 1) < fn.factor(mid) < 1.0
    assert fn.factor(total) == low and fn.factor(total + 5) == low
    factors = [fn.factor(t) for t in range(total + 6)]
    assert all(a < b for a, b in zip(factors[:warmup - 1], factors[1:warmup]))  # strictly up through the warm-up
    assert all(a >= b for a, b in zip(factors[warmup:], factors[warmup + 1:]))  # never up again
    # min_factor defaults to 0; a schedule without a cosine part (total == warmup) does not divide by zero
    assert WarmupCosineLRFn(2, 4).factor(4) == 0.0 and WarmupCosineLRFn(2, 4).factor(3) == pytest.approx(0.5)
    assert WarmupCosineLRFn(3, 3).factor(2) == 1.0 and WarmupCosineLRFn(3, 3).factor(3) == 0.0


def test_step_decay_boundaries():
    from mmvae_amd.modules.base import StepDecayLRFn

    fn = StepDecayLRFn(step_size=4, gamma=0.5)
    assert [fn.factor(t) for t in (0, 3, 4, 7, 8, 12)] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.125]
    fn = StepDecayLRFn("1e1", "0.1")  # as PyYAML hands `1e1` over
    assert fn.step_size == 10 and isinstance(fn.step_size, int) and fn.factor(9) == 1.0
    assert fn.factor(10) == pytest.approx(0.1) and fn.factor(25) == pytest.approx(0.01)


def test_schedules_count_their_own_steps():
    from mmvae_amd.modules.base import WarmupCosineLRFn

    fn = WarmupCosineLRFn(5, 20)
    assert fn.step_count == 0
    fn.step(), fn.step()
    assert fn.step_count == 2
    fn.step_count = 11  # a resumed run
    fn.step()
    assert fn.step_count == 12


_MODEL_NODE = """
class_path: cmmvae.models.CMMVAEModel
init_args:
  kl_annealing_fn:
    class_path: cmmvae.modules.base.KLAnnealingFn
    init_args: {kl_weight: 1.0}
  lr_schedule_fn:
    class_path: cmmvae.modules.base.WarmupCosineLRFn
    init_args: {warmup_steps: 1e1, total_steps: 40}
  optim_cls: AdamW
  module:
    class_path: cmmvae.modules.CMMVAE
    init_args:
      vae:
        class_path: cmmvae.modules.CLVAE
        init_args:
          latent_dim: 4
          encoder_config:
            class_path: cmmvae.modules.base.FCBlockConfig
            init_args: {layers: [8, 6], dropout_rate: 0.0, use_batch_norm: true, use_layer_norm: false,
                        activation_fn: torch.nn.ReLU, return_hidden: true}
          decoder_config:
            class_path: cmmvae.modules.base.FCBlockConfig
            init_args: {layers: [4, 6, 8], dropout_rate: 0.0, use_batch_norm: false, use_layer_norm: false,
                        activation_fn: torch.nn.ReLU}
      experts:
        class_path: cmmvae.modules.base.Experts
        init_args:
          experts:
          - class_path: cmmvae.modules.base.Expert
            init_args:
              id: human
              encoder_config:
                class_path: cmmvae.modules.base.FCBlockConfig
                init_args: {layers: [21, 8], dropout_rate: 0.0, use_batch_norm: true, use_layer_norm: false,
                            activation_fn: torch.nn.ReLU}
              decoder_config:
                class_path: cmmvae.modules.base.FCBlockConfig
                init_args: {layers: [8, 21], dropout_rate: 0.0, use_batch_norm: false, use_layer_norm: false,
                            activation_fn: torch.nn.ReLU}
          - class_path: cmmvae.modules.base.Expert
            init_args:
              id: mouse
              encoder_config:
                class_path: cmmvae.modules.base.FCBlockConfig
                init_args: {layers: [17, 8], dropout_rate: 0.0, use_batch_norm: true, use_layer_norm: false,
                            activation_fn: torch.nn.ReLU}
              decoder_config:
                class_path: cmmvae.modules.base.FCBlockConfig
                init_args: {layers: [8, 17], dropout_rate: 0.0, use_batch_norm: false, use_layer_norm: false,
                            activation_fn: torch.nn.ReLU}
"""


def test_yaml_node_with_schedule_and_adamw_builds_hip_optimisers():
    from mmvae_amd import backend, instantiate
    from mmvae_amd.modules.base import WarmupCosineLRFn
    from mmvae_amd.optim import HipAdam

    node = yaml.safe_load(_MODEL_NODE)
    assert node["init_args"]["lr_schedule_fn"]["init_args"]["warmup_steps"] == "1e1"  # a string to PyYAML
    with backend.cpu_plumbing():
        model = instantiate.build(node)
        optimizers = model.configure_optimizers()
    fn = model.lr_schedule_fn
    assert isinstance(fn, WarmupCosineLRFn)
    assert fn.warmup_steps == 10 and isinstance(fn.warmup_steps, int) and fn.total_steps == 40 and fn.min_factor == 0.0
    assert fn.factor(0) == pytest.approx(0.1) and fn.factor(9) == 1.0
    assert model.optim_cls == "AdamW" and len(optimizers) == 3
    assert all(isinstance(o, HipAdam) and o.decoupled_weight_decay for o in optimizers)
    assert all(o.param_groups[0]["lr"] == 5e-3 and o.param_groups[0]["weight_decay"] == 1e-6 for o in optimizers)
    assert "decoupled_weight_decay" not in optimizers[0].state_dict()["param_groups"][0]  # torch's keys only
    assert [float(v) for v in optimizers[0].hyper_dev] == [pytest.approx(5e-3), pytest.approx(1e-6), 1.0, 0.0]
    assert all(k.startswith("module.") for k in model.state_dict())
    # the argument wins over the constructor's choice; "Adam" stays coupled
    with backend.cpu_plumbing():
        coupled = instantiate.build(yaml.safe_load(_MODEL_NODE)).configure_optimizers("Adam")
    assert all(isinstance(o, HipAdam) and not o.decoupled_weight_decay for o in coupled)


def test_schedule_sets_every_optimisers_lr_before_each_step():
    """Three steps of golden case two_mod_odd on CPU plumbing with a warm-up schedule: while step t runs, every
    optimiser's lr is 5e-3 x factor(t) -- also those of the experts that do not train in that step -- and lr/training
    is logged; without a schedule nothing is."""
    from mmvae_amd.modules.base import KLAnnealingFn, WarmupCosineLRFn

    seen = []

    class Probe(KLAnnealingFn):  # its step() runs inside training_step, behind the optimisers' updates
        def __init__(self, model):
            super().__init__(1.0)
            self.model = model

        def step(self):
            seen.append([o.param_groups[0]["lr"] for o in self.model.optimizers()])

    def prepare(model):
        model.lr_schedule_fn = WarmupCosineLRFn(3, 5, min_factor=0.25)  # moves on every one of the three steps
        model.kl_annealing_fn = Probe(model)

    case, _, results = MU.replay_training("two_mod_odd", "cpu", prepare=prepare)
    steps = len(case["schedule"])
    assert steps == 3 and len(seen) == steps
    fn = WarmupCosineLRFn(3, 5, min_factor=0.25)
    factors = [fn.factor(t) for t in range(steps)]
    assert factors == [1 / 3, 2 / 3, 1.0]
    for t, (lrs, r) in enumerate(zip(seen, results)):
        assert len(lrs) == 3 and all(lr == 5e-3 * factors[t] for lr in lrs), (t, lrs)
        assert r["logged"]["lr/training"] == 5e-3 * factors[t]
    _, _, plain = MU.replay_training("two_mod_odd", "cpu")
    assert not any(k.startswith("lr/") for r in plain for k in r["logged"])
    # the schedule changed the run
    assert H.rel_l2(results[-1]["sd"]["vae.decoder.fc_layers.0.lin.weight"],
                    plain[-1]["sd"]["vae.decoder.fc_layers.0.lin.weight"]) > 1e-5


def _rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def test_decoupled_hip_adam_is_torch_adamw_on_cpu_plumbing():
    """HipAdam(decoupled_weight_decay=True) against torch.optim.AdamW over two steps with the 10.0 norm clip
    (n = 70 001, the gradients of tests/test_kernels_gpu.py::test_clip_adam_matches_torch).  weight_decay = 1e-2: at the
    default 1e-6, 1 - lr * wd rounds to 1 in fp32 and the two decay rules could not be told apart.  Bounds: parameters
    rel-L2 1e-6, moments 5e-5 (torch's clip coefficient comes from an fp32 norm); the coupled rule on the same run sits
    more than 1e-4 away, so the comparison is not vacuous."""
    from mmvae_amd import backend
    from mmvae_amd.optim import HipAdam

    n = 70001
    p0, grads = _rnd(n, 1), (_rnd(n, 2, 3.0), _rnd(n, 3, 0.001))
    pt = torch.nn.Parameter(p0.clone())
    ref = torch.optim.AdamW([pt], lr=5e-3, weight_decay=1e-2)
    with backend.cpu_plumbing():
        pd_, pc = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
        dec = HipAdam([pd_], lr=5e-3, weight_decay=1e-2, decoupled_weight_decay=True)
        cpl = HipAdam([pc], lr=5e-3, weight_decay=1e-2)
        assert dec.decoupled_weight_decay and not cpl.decoupled_weight_decay
        for g in grads:
            pt.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([pt], 10.0)
            ref.step()
            for opt, p in ((dec, pd_), (cpl, pc)):
                opt.zero_grad()
                p.grad = g.clone()
                opt.set_clip(10.0)
                opt.step()
    print("decoupled vs AdamW: p", H.rel_l2(pd_.detach(), pt.detach()), "m",
          H.rel_l2(dec.arena.exp_avg[:n], ref.state[pt]["exp_avg"]), "v",
          H.rel_l2(dec.arena.exp_avg_sq[:n], ref.state[pt]["exp_avg_sq"]), "| coupled vs decoupled: p",
          H.rel_l2(pc.detach(), pd_.detach()))
    assert H.rel_l2(pd_.detach(), pt.detach()) < 1e-6
    assert H.rel_l2(dec.arena.exp_avg[:n], ref.state[pt]["exp_avg"]) < 5e-5
    assert H.rel_l2(dec.arena.exp_avg_sq[:n], ref.state[pt]["exp_avg_sq"]) < 5e-5
    assert H.rel_l2(pc.detach(), pd_.detach()) > 1e-4
