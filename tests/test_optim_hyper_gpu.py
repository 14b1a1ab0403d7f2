"""The optimiser's learning rate, weight decay and decay mode as device words (`_hp` entry points of include/mmvae_hip.h,
HipAdam.hyper_dev): bit-identity with the recorded results of the retired by-value entries in coupled mode,
torch.optim.AdamW's rule in decoupled mode, a captured graph that follows the words, and the step engine under per-step
schedules -- against the module path, without rebuilding its programs, with `optim_cls="AdamW"` models taken by the
engine, and on the sharded update."""
import os
import tempfile
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import mirror_utils as MU  # noqa: E402

LR, WD, B1, B2, EPS, GS = 5e-3, 1e-2, 0.9, 0.999, 1e-8, 0.5


def _rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from mmvae_amd import _lib

    lib = _lib.load()
    assert lib.mmvae_abi_version() >= 13
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _state(cv=0.0):
    return torch.tensor([4.0, 0, 0.7, 0.9, 0.95, cv, 0, 0], device="cuda")  # step, norm, clip, bias corrections, clip value


def _hyper(lr=LR, wd=WD, decoupled=0.0):
    return torch.tensor([lr, wd, decoupled, 0.0], device="cuda")


def _arenas(n, offset=0, pad=8):
    """p, g, m, v of n floats starting `offset` floats into 16-byte-aligned allocations (the same numbers at any offset)."""
    out = []
    for seed, scale, absolute in ((1, 1.0, False), (2, 0.1, False), (3, 0.01, False), (4, 0.01, True)):
        full = torch.zeros(n + pad, device="cuda")
        vals = _rnd(n, seed, scale)
        full[offset:offset + n] = (vals.abs() if absolute else vals).cuda()
        out.append(full)
    return out


def _views(full, n, offset):
    return [t[offset:offset + n] for t in full]


# The by-value entry points (the step, its copy rider, the job list and the multi-arena launch with lr and weight decay
# as launch arguments) left the library with ABI 14.  What they produced at ABI 13 for exactly the inputs built below is
# recorded in tests/golden/adam_by_value.npz (tests/golden/make_adam_golden.py, which also proved the ABI 13 `_hp`
# entries bit-identical to them in the same run).
JOB_N = 50_000
JOB_SEGS = [(0, 1, 0), (5, 16384, 0), (16392, 100, 2), (16500, 16384, 0), (40_000, 4099, 0)]  # offset, len, flag
MULTI_SIZES = [(4099, 0, 5e-3, 1e-2), (1027, 1, 1e-3, 0.0)]  # n, offset, lr, weight decay
MULTI_CV = (0.0, 0.05)


def _job_table():
    from mmvae_amd.optim import HipAdam

    jobs = np.zeros(len(JOB_SEGS), dtype=np.dtype(HipAdam.JOB_DTYPE))
    for j, (o, ln, f) in enumerate(JOB_SEGS):
        assert o + ln <= JOB_N
        jobs[j]["offset"], jobs[j]["len"], jobs[j]["bc1"], jobs[j]["bc2"], jobs[j]["reserved"] = o, ln, 0.1 + 0.1 * j, 0.001 * (j + 1), f
    return torch.from_numpy(jobs.view(np.uint8)).cuda()


@pytest.fixture(scope="module")
def by_value():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_by_value.npz")) as z:
        out = {k: torch.from_numpy(z[k]).cuda() for k in z.files}
    assert all(t.dtype == torch.float32 for t in out.values())
    return out


@pytest.mark.parametrize("n,offset", [(4099, 0), (4099, 1), (3, 0)], ids=["vector+tail", "scalar", "n3"])
@pytest.mark.parametrize("cv", [0.0, 0.05], ids=["norm", "value"])
def test_hp_equals_by_value_bit_for_bit(lib, by_value, n, offset, cv):
    """hyper = {lr, wd, 0, 0}: the recorded bits of the by-value step -- 16-byte body + 3-element tail, the scalar path of
    unaligned arenas (a record of its own: the two loops do not round alike), fewer elements than one
    16-byte group -- and nothing written outside [0, n)."""
    state = _state(cv)
    got = _arenas(n, offset)
    p, g, m, v = _views(got, n, offset)
    assert (p.data_ptr() % 16 == 0) == (offset == 0)
    assert lib.mmvae_adam_step_hp(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(),
                                  _hyper().data_ptr(), B1, B2, EPS, GS, _stream()) == 0
    torch.cuda.synchronize()
    fresh = _arenas(n, offset)
    for name, t in zip("pmv", (p, m, v)):
        assert torch.equal(t, by_value[f"step_n{n}_off{offset}_cv{cv:g}_{name}"]), name
    assert not torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])  # it stepped; the gradient is read only
    for t, f in zip(got, fresh):  # the padding around the arena is untouched
        assert torch.equal(t[:offset], f[:offset]) and torch.equal(t[offset + n:], f[offset + n:])


def test_hp_copy_rider_and_confined_grid_equal_by_value(lib, by_value):
    """mmvae_adam_step_copy_hp on the chip-filling grid and on 7 fat workgroups (mmvae_adam_set_workgroups): the recorded
    bits of the by-value step (its rider form gave the same), and the rider's words copied."""
    n = 4099
    state = _state()
    src = _rnd(256, 5).cuda()
    outs = []
    try:
        for wg in (0, 7):
            assert lib.mmvae_adam_set_workgroups(wg) == 0
            p, g, m, v = _arenas(n)
            dst = torch.zeros(256, device="cuda")
            assert lib.mmvae_adam_step_copy_hp(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(),
                                               _hyper().data_ptr(), B1, B2, EPS, GS, 256, src.data_ptr(), dst.data_ptr(),
                                               _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(dst, src), wg
            assert torch.equal(g, _arenas(n)[1]), wg
            outs.append((p, m, v))
    finally:
        lib.mmvae_adam_set_workgroups(0)
    for out in outs:
        for name, t in zip("pmv", out):
            assert torch.equal(t[:n], by_value[f"step_n{n}_off0_cv0_{name}"]), name
            assert torch.equal(t, outs[0]["pmv".index(name)])  # confined grid == chip-filling grid, padding included
    assert not torch.equal(outs[0][0], _arenas(n)[0])


def test_hp_jobs_equal_by_value(lib, by_value):
    """mmvae_adam_step_jobs_hp: jobs at offsets 0 (16-byte path) and 5 (scalar path), lengths 1 and 16 384, a full
    aligned job and a retired one -- the recorded bits of the by-value job launch; retired and unlisted elements
    untouched."""
    n = JOB_N
    jobs_dev = _job_table()
    state = _state()
    got = _arenas(n)
    p, g, m, v = got
    assert lib.mmvae_adam_step_jobs_hp(len(JOB_SEGS), jobs_dev.data_ptr(), p.data_ptr(), g.data_ptr(), m.data_ptr(),
                                       v.data_ptr(), state.data_ptr(), _hyper().data_ptr(), B1, B2, EPS, GS, _stream()) == 0
    torch.cuda.synchronize()
    for name, t in zip("pmv", (p, m, v)):
        assert torch.equal(t[:n], by_value[f"jobs_{name}"]), name
    fresh = _arenas(n)
    assert torch.equal(g, fresh[1])
    touched = torch.zeros(n + 8, dtype=torch.bool, device="cuda")
    for o, ln, f in JOB_SEGS:
        if f != 2:
            touched[o:o + ln] = True
    for t, f in zip((got[0], got[2], got[3]), (fresh[0], fresh[2], fresh[3])):
        assert torch.equal(t[~touched], f[~touched])
        assert not (t[touched] == f[touched]).all()


def test_hp_multi_equals_by_value(lib, by_value):
    """mmvae_adam_step_multi_hp over two arenas (one unaligned, each with its own hyper words) against the recorded bits
    of the by-value multi-arena launch."""
    import ctypes as C

    from mmvae_amd import _lib

    sizes = MULTI_SIZES
    states = [_state(cv) for cv in MULTI_CV]
    hypers = [_hyper(lr, wd) for _, _, lr, wd in sizes]
    arenas = [_arenas(n, off) for n, off, _, _ in sizes]
    table = (_lib.AdamArenaHp * len(sizes))()
    for e, full, (n, off, lr, wd), st, hy in zip(table, arenas, sizes, states, hypers):
        p, g, m, v = _views(full, n, off)
        e.p, e.g, e.m, e.v, e.state, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), n
        e.beta1, e.beta2, e.eps, e.grad_scale = B1, B2, EPS, GS
        e.hyper = hy.data_ptr()
    raw = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    assert C.sizeof(table) == raw.numel()
    assert lib.mmvae_adam_step_multi_hp(len(sizes), raw.data_ptr(), max(n for n, _, _, _ in sizes), _stream()) == 0
    torch.cuda.synchronize()
    for k, (got, (n, off, _, _)) in enumerate(zip(arenas, sizes)):
        fresh = _arenas(n, off)
        p, g, m, v = _views(got, n, off)
        for name, t in zip("pmv", (p, m, v)):
            assert torch.equal(t, by_value[f"multi{k}_{name}"]), (k, name)
        assert not torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
        for t, f in zip(got, fresh):  # nothing written around the arena
            assert torch.equal(t[:off], f[:off]) and torch.equal(t[off + n:], f[off + n:])


def test_hp_entries_reject_bad_arguments(lib):
    p, g, m, v = _arenas(16)
    st, hy = _state(), _hyper()
    ptrs = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr()]
    assert lib.mmvae_adam_step_hp(16, *ptrs, None, B1, B2, EPS, GS, _stream()) == 1
    assert lib.mmvae_adam_step_hp(0, *ptrs, hy.data_ptr(), B1, B2, EPS, GS, _stream()) == 1
    assert lib.mmvae_adam_step_copy_hp(16, *ptrs, None, B1, B2, EPS, GS, 0, None, None, _stream()) == 1
    assert lib.mmvae_adam_step_copy_hp(16, *ptrs, hy.data_ptr(), B1, B2, EPS, GS, 4, None, None, _stream()) == 1
    assert lib.mmvae_adam_step_jobs_hp(1, st.data_ptr(), *ptrs, None, B1, B2, EPS, GS, _stream()) == 1
    assert lib.mmvae_adam_step_multi_hp(0, st.data_ptr(), 16, _stream()) == 1
    assert lib.mmvae_adam_step_multi_hp(1, None, 16, _stream()) == 1
    torch.cuda.synchronize()
    assert torch.equal(p, _arenas(16)[0])


@pytest.mark.parametrize("clip", ["norm", "value"])
def test_decoupled_matches_fp64_adamw(lib, clip):
    """decoupled = 1 against torch.optim.AdamW in fp64 (lr 5e-3, weight decay 1e-2: at the default 1e-6, 1 - lr * wd
    rounds to 1 in fp32), two steps, global-norm clip at 10 and clip by value at 0.05.  Bounds of
    test_clip_adam_matches_torch: parameters rel-L2 1e-6, moments 5e-5; the coupled rule sits far outside them."""
    from mmvae_amd import ops

    n, cv = 70001, 0.05
    p0, grads = _rnd(n, 1), (_rnd(n, 2, 3.0), _rnd(n, 3, 0.001))
    pt = torch.nn.Parameter(p0.double())
    ref = torch.optim.AdamW([pt], lr=LR, weight_decay=WD)
    runs = {}
    for name, dec in (("decoupled", 1.0), ("coupled", 0.0)):
        runs[name] = dict(p=p0.clone().cuda(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"),
                          state=torch.zeros(8, device="cuda"), hyper=_hyper(LR, WD, dec))
        if clip == "value":
            runs[name]["state"][5] = cv
    partials = torch.empty(ops.sqnorm_partials(n), device="cuda")
    for g in grads:
        pt.grad = g.double()
        if clip == "norm":
            torch.nn.utils.clip_grad_norm_([pt], 10.0)
        else:
            torch.nn.utils.clip_grad_value_([pt], cv)
        ref.step()
        for r in runs.values():
            ops.clip_adam_step(r["p"], g.cuda(), r["m"], r["v"], r["state"], partials,
                               max_norm=10.0 if clip == "norm" else 0.0, hyper=r["hyper"])
    d, c = runs["decoupled"], runs["coupled"]
    errs = (H.rel_l2(d["p"], pt.detach()), H.rel_l2(d["m"], ref.state[pt]["exp_avg"]),
            H.rel_l2(d["v"], ref.state[pt]["exp_avg_sq"]))
    print(f"decoupled vs fp64 AdamW ({clip}): p {errs[0]:.3g} m {errs[1]:.3g} v {errs[2]:.3g}; "
          f"coupled vs AdamW: p {H.rel_l2(c['p'], pt.detach()):.3g}")
    assert float(d["state"][0]) == 2.0
    assert errs[0] < 1e-6 and errs[1] < 5e-5 and errs[2] < 5e-5
    assert H.rel_l2(c["p"], pt.detach()) > 1e-4


def test_captured_graph_follows_the_device_words(lib):
    """One captured single-stream graph of mmvae_adam_step_hp (n = 4 099), replayed twice with `hyper` rewritten in
    between (another lr, then the decoupled mode): each replay leaves the bits of an eager launch with that replay's
    values -- the graph holds the address, not the numbers."""
    n = 4099
    state = _state()
    settings = [(LR, WD, 0.0), (1e-3, WD, 0.0), (2e-3, 3e-2, 1.0)]

    def eager():
        p, g, m, v = _arenas(n)
        for lr, wd, dec in settings:
            assert lib.mmvae_adam_step_hp(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(),
                                          _hyper(lr, wd, dec).data_ptr(), B1, B2, EPS, GS, _stream()) == 0
            torch.cuda.synchronize()
            yield p.clone(), m.clone(), v.clone()

    want = list(eager())
    p, g, m, v = _arenas(n)
    hyper = _hyper(*settings[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = lib.mmvae_adam_step_hp(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(),
                                        hyper.data_ptr(), B1, B2, EPS, GS, _stream())
    assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for (lr, wd, dec), (wp, wm, wv) in zip(settings, want):
        hyper[0:1].fill_(lr), hyper[1:2].fill_(wd), hyper[2:3].fill_(dec)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(p, wp) and torch.equal(m, wm) and torch.equal(v, wv), (lr, wd, dec)
    # the second replay did not repeat the first one's step size
    p2 = _arenas(n)
    for _ in range(2):
        assert lib.mmvae_adam_step_hp(n, p2[0].data_ptr(), p2[1].data_ptr(), p2[2].data_ptr(), p2[3].data_ptr(),
                                      state.data_ptr(), _hyper(*settings[0]).data_ptr(), B1, B2, EPS, GS, _stream()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(p2[0], want[1][0])


# ----------------------------------------------------------------------------------------- engine against module path
LRS = [4e-3, 2.5e-3, 1e-3]


def _prepare(optim_cls, schedule):
    def prepare(model):
        from mmvae_amd.modules.base import WarmupCosineLRFn

        model.optim_cls = optim_cls
        if schedule:
            model.lr_schedule_fn = WarmupCosineLRFn(3, 5, min_factor=0.25)  # 1/3, 2/3, 1: another lr on every step

    return prepare


def _edit(schedule):
    def edit(model, t):
        for o in model.optimizers():
            if not schedule:
                o.param_groups[0]["lr"] = LRS[t]
            if t == 1:
                o.param_groups[0]["weight_decay"] = 1e-2

    return edit


def _assert_same_training(ra, rb, lr_ratio=1.0):
    """Bounds of test_step_gpu.py::test_engine_follows_settings_changed_after_capture: parameters 1e-5, running_mean
    5e-5, loss 2e-5.  That test -- and the schedules of this file -- take every step after the first at lr <= 2.5e-3
    (1e-3 there).  The distance between the two paths comes from an expert's COLD Adam step (mouse's first, at t = 1):
    with zero moments the update is lr * g / (|g| + eps), sign-like, so an element whose gradient sits at rounding
    level moves by up to +-lr on either path whatever the gradients' agreement (tests/mirror_utils.py says the same of
    the oracle comparison) -- the parameter distance is linear in that step's lr.  `lr_ratio`: the lr of a run's cold
    steps over the 1e-3 those bounds were set at, for runs that keep the constant 5e-3; parameter bounds scale with it."""
    assert len(ra) == len(rb) > 0
    for a, b in zip(ra, rb):
        for k, v in a["sd"].items():
            if v.is_floating_point() and not k.endswith("lin.bias"):
                tol = (5e-5 if k.endswith("running_mean") else 1e-5) * lr_ratio
                assert H.rel_l2(v, b["sd"][k]) < tol, (k, H.rel_l2(v, b["sd"][k]))
        la, lb = a["logged"][f"loss/training/{a['eid']}"], b["logged"][f"loss/training/{b['eid']}"]
        assert abs(la - lb) <= 2e-5 * abs(lb)


@pytest.mark.parametrize("schedule", [False, True], ids=["param_groups", "lr_schedule_fn"])
@pytest.mark.parametrize("optim_cls", ["Adam", "AdamW"])
@pytest.mark.parametrize("name", ["two_mod_odd", "adversarial", "cond_par"])
def test_engine_follows_a_per_step_schedule_like_the_module_path(name, optim_cls, schedule):
    """lr rewritten before EVERY step (through param_groups, or by the model's lr_schedule_fn) and weight_decay once:
    the captured programs read the device words and stay with the module path; cond_par steps through the jobs kernel."""
    from mmvae_amd.optim import HipAdam

    results = {}
    for use_engine in (True, False):
        _, _, results[use_engine] = MU.replay_training(name, "cuda", use_engine=use_engine,
                                                       prepare=_prepare(optim_cls, schedule), before_step=_edit(schedule))
        engine = MU.replay_training.last_engine
        assert bool(engine) == use_engine
        if use_engine:
            opts = engine.model.optimizers()
            assert all(isinstance(o, HipAdam) and o.decoupled_weight_decay == (optim_cls == "AdamW") for o in opts)
            assert engine._sig_changes == 0  # no settings-signature rebuild
            last = results[True][-1]["eid"]  # the words of the optimisers the last step stepped are that step's
            stepped = [engine.opts["vae"], engine.opts["experts"][last]] + list((engine.opts.get("adversarials") or {}).values())
            for o in stepped:
                g = o.param_groups[0]
                assert o.hyper_dev.tolist() == pytest.approx([g["lr"], 1e-2, float(optim_cls == "AdamW"), 0.0], rel=1e-6)
    _assert_same_training(results[True], results[False])
    if schedule:
        steps = len(results[True])
        for r in results.values():
            assert [x["logged"]["lr/training"] for x in r] == pytest.approx([5e-3 * f for f in (1 / 3, 2 / 3, 1.0)][:steps])


def test_adamw_model_is_taken_by_the_engine():
    """optim_cls="AdamW": decline_reason is None, no "does not cover" warning, the engine's steps are the module path's,
    and they are not the coupled optimiser's (weight decay 1e-2 from the first step on).  The run keeps the constant
    lr 5e-3, five times the 1e-3 at which the borrowed parameter bounds were set (_assert_same_training): 5e-5 here.
    Measured at the 1e-5 of lr 1e-3: experts.mouse.encoder.fc_layers.0.lin.weight 1.17e-5 after mouse's cold step."""
    from mmvae_amd.engine import StepEngine

    def prepare(cls):
        def fn(model):
            model.optim_cls = cls
            for o in model.optimizers():
                o.param_groups[0]["weight_decay"] = 1e-2
            if model.use_engine:
                assert StepEngine.decline_reason(model) is None

        return fn

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, _, ra = MU.replay_training("two_mod_odd", "cuda", use_engine=True, prepare=prepare("AdamW"))
        assert MU.replay_training.last_engine
    assert not [w for w in caught if "does not cover" in str(w.message)]
    _, _, rb = MU.replay_training("two_mod_odd", "cuda", use_engine=False, prepare=prepare("AdamW"))
    _assert_same_training(ra, rb, lr_ratio=5.0)
    _, _, rc = MU.replay_training("two_mod_odd", "cuda", use_engine=True, prepare=prepare("Adam"))
    k = "vae.decoder.fc_layers.0.lin.weight"
    assert H.rel_l2(ra[-1]["sd"][k], rc[-1]["sd"][k]) > 1e-5


# ------------------------------------------------------------------------------------------------------- no rebuild
def _run(name, prepare, before_step, extra_steps=0):
    """The golden schedule of `name` (+ `extra_steps` more, reusing the inputs from the start) through the engine, every
    batch a tensor of its own that stays alive (no pointer is seen twice: every step reads the static input buffer).
    Returns (model, the plan that served each step, number of plans after each step)."""
    case, z = H.load_case(name)
    keep, plans, counts = [], [], []
    T = len(case["schedule"])
    with tempfile.TemporaryDirectory() as tmpdir:
        model = MU.build_mirror(case, "cuda", tmpdir, use_engine=True)
        MU.load_state(model, z, "sd0/")
        model.train()
        model.trainer.set_stage("training")
        prepare(model)
        for t in range(T + extra_steps):
            eid = case["schedule"][t % T]
            x, eps, masks, labels = H.step_inputs(z, t % T)
            before_step(model, t)
            model.kl_annealing_fn.kl_weight = case["kl_weights"][t % T]
            model.module.vae.encoder.explicit_eps = eps.cuda()
            MU.set_explicit_masks(model, masks, eid, "cuda")
            keep.append(x.cuda())
            model.training_step((keep[-1], pd.DataFrame({"dummy": [0] * x.shape[0]}), eid), t)
            plans.append(model._engine.last_plan)
            counts.append(len(model._engine._plans))
        torch.cuda.synchronize()
    return model, plans, counts


def test_schedule_does_not_rebuild_the_captured_programs(monkeypatch):
    """two_mod_odd trains human, mouse, human: with another lr on every step (lr_schedule_fn) and a weight_decay edit no
    plan is released, the plan of the first human step serves the second, and there are as many plans as at constant
    lr; new betas in the same run still drop and rebuild the programs."""
    from mmvae_amd import engine as E
    from mmvae_amd.modules.base import WarmupCosineLRFn

    released = []
    release = E._Plan.release
    monkeypatch.setattr(E._Plan, "release", lambda self: (released.append(self), release(self))[1])

    def scheduled(model):
        model.lr_schedule_fn = WarmupCosineLRFn(3, 5)

    def edit(model, t):
        if t == 1:
            for o in model.optimizers():
                o.param_groups[0]["weight_decay"] = 1e-3
        if t == 3:
            assert not released  # three steps, three learning rates: nothing was dropped
            for o in model.optimizers():
                o.param_groups[0]["betas"] = (0.8, 0.99)

    _, const_plans, const_counts = _run("two_mod_odd", lambda model: None, lambda model, t: None)
    assert not released and const_plans[0] is const_plans[2] and const_plans[0] is not const_plans[1]
    model, plans, counts = _run("two_mod_odd", scheduled, edit, extra_steps=1)
    lrs = [5e-3 * f for f in (1 / 3, 2 / 3, 1.0)]
    assert model.lr_schedule_fn.step_count == 4
    assert plans[0] is plans[2] and plans[0] is not plans[1]
    assert counts[:3] == const_counts
    assert lrs[0] != lrs[2]  # the shared plan ran at two learning rates
    # step 3 (human again) came with new betas: the training plans were released and human's was built anew
    assert released and all(p in released for p in plans[:3])
    assert plans[3] is not plans[0] and plans[3].eid == plans[0].eid
    assert model._engine._sig_changes == 1


# ------------------------------------------------------------------------------------------------- sharded update
def test_sharded_update_follows_the_schedule_with_single_rank_rccl():
    """The sharded expert update (reduce-scatter, Adam on the slice through mmvae_adam_step_hp, all-gather) with a real
    one-rank process group, AdamW and a per-step schedule, against the unsharded update (MMVAE_DP_SHARD=0): 2e-6, the
    bound of test_dist_gpu.py's sharded-against-all-reduce test.  In a child process (tests.helpers.run_in_child)."""
    H.run_in_child("tests.test_optim_hyper_gpu", "_body_sharded_schedule",
                   {"MMVAE_SINGLE_RANK_COLLECTIVES": "1", "MASTER_PORT": "29633", "MASTER_ADDR": "127.0.0.1"})


def _body_sharded_schedule():
    import torch.distributed as td

    from mmvae_amd import dist as mdist

    mdist.init_from_env()
    try:
        assert mdist.collectives_active()
        sharded = []

        def prepare(model):
            _prepare("AdamW", True)(model)
            model.optimizers()
            mdist.broadcast_parameters(model)
            mdist.attach(model)

        def edit(model, t):
            _edit(True)(model, t)
            if t > 0:
                sharded.append(any(o.sharded for o in model.optimizers()))

        runs = {}
        for shard in ("1", "0"):
            os.environ["MMVAE_DP_SHARD"] = shard
            _, _, runs[shard] = MU.replay_training("two_mod_odd", "cuda", use_engine=True, prepare=prepare, before_step=edit)
            assert MU.replay_training.last_engine and MU.replay_training.last_engine._sig_changes == 0
        assert sharded == [True, True, False, False], sharded
        for a, b in zip(runs["1"], runs["0"]):
            for k, v in a["sd"].items():
                if v.is_floating_point():
                    assert H.rel_l2(v, b["sd"][k]) < 2e-6, (k, H.rel_l2(v, b["sd"][k]))
        print("CHILD_CASE_OK", flush=True)
    finally:
        torch.cuda.synchronize()
        td.destroy_process_group()
