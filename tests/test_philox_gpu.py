"""The device generator (mmvae_philox_* of csrc/elbo_optim.hip) against its host mirror (tests/philox_mirror.py, held to
the published Philox4x32-10 known answers by tests/test_philox_mirror.py): keep masks bit for bit, normals within a bound
that follows the Box-Muller radius, the counter's advance (single fills, the ticketed job launch, eager and captured),
and the numbers a production-mode engine step really draws.  Plus two small kernels of the same file that had no direct
test: mmvae_sum_rows_f32 and both variants of mmvae_axpby."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import philox_mirror as M  # noqa: E402

U64 = (1 << 64) - 1
STREAM_DROPOUT, STREAM_NORMAL = 0x44524F50, 0x4E4F524D  # mmvae_amd.rng (asserted equal in the engine test)

# (seed, offset, stream id): zeros; the carry into the high counter word inside the draw, with the stream's high word in
# use and an all-ones seed; an offset above 2^63 (a negative int64 in the state tensor) on the dropout stream
STATES = [(0, 0, 0), (U64, 2 ** 32 - 3, 2 ** 32 + 7), (1234, 2 ** 63 + 5, STREAM_DROPOUT)]
NS = [1, 3, 4, 5, 1023, 2097157]  # the last: 2048 workgroups x 256 threads x 4 elements + 5 -> grid-stride loop + a tail
PS = [0.0, 2.0 ** -25, 0.1, 0.5, 1.0 - 2.0 ** -23]

# |got - mirror| <= NORMAL_C * 2^-23 * max(r, 2^-12), r = the mirror's Box-Muller radius of the element.  The largest ratio
# measured on the MI355X over every normal case of this file is 1.738 (the 2 097 157-element fill from seed 0, offset 0,
# stream 0); the bound is twice that.  Above 16 the documented ulp bounds of the device's logf / sqrtf / sincosf would not
# explain the error: a larger constant here is a finding, not a setting.
NORMAL_MEASURED = 1.738
NORMAL_C = 2.0 * NORMAL_MEASURED
assert NORMAL_C <= 16.0

GUARD_BYTE, GUARD_FLOAT = 0xAB, -777.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from mmvae_amd import _lib

    return _lib.load()


def _i64(v):
    v &= U64
    return v - (1 << 64) if v >= (1 << 63) else v


def _state(seed, offset):
    return torch.tensor([_i64(seed), _i64(offset)], dtype=torch.int64, device="cuda")


def _read(rng_t):
    return [int(v) & U64 for v in rng_t.tolist()]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _mask_buf(n):
    return torch.full((n + 64,), GUARD_BYTE, dtype=torch.uint8, device="cuda")


def _float_buf(n):
    return torch.full((n + 16,), GUARD_FLOAT, dtype=torch.float32, device="cuda")


def _assert_mask(buf, n, want, what):
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got[:n] != want)
    assert bad.size == 0, f"{what}: {bad.size} of {n} mask bytes differ, first at {int(bad[0])}"
    assert bool((got[n:] == GUARD_BYTE).all()), f"{what}: guard bytes behind the mask were written"


def _assert_normal(buf, n, want, radius, what):
    """Returns the largest |got - mirror| / (2^-23 max(r, 2^-12))."""
    got = buf.cpu().numpy()
    assert bool((got[n:] == np.float32(GUARD_FLOAT)).all()), f"{what}: guard floats behind the fill were written"
    assert bool(np.isfinite(got[:n]).all()), f"{what}: non-finite normals"
    ratio = np.abs(got[:n].astype(np.float64) - want) / (2.0 ** -23 * np.maximum(radius, 2.0 ** -12))
    worst = float(ratio.max())
    print(f"philox normal {what}: max ratio {worst:.3f}")
    assert worst <= NORMAL_C, f"{what}: ratio {worst} at element {int(ratio.argmax())} (bound {NORMAL_C})"
    return worst


# ------------------------------------------------------------------------------------------------- single fills
@pytest.mark.parametrize("state", range(len(STATES)))
@pytest.mark.parametrize("n", NS)
def test_keep_mask_equals_mirror(lib, n, state):
    seed, off, stream = STATES[state]
    rng_t = _state(seed, off)
    for p in PS:
        buf = _mask_buf(n)
        assert lib.mmvae_philox_keep_mask(n, p, buf.data_ptr(), rng_t.data_ptr(), stream, 0, _s()) == 0
        _assert_mask(buf, n, M.keep_mask(n, p, seed, off, stream), f"n={n} p={p} state={state}")
    assert _read(rng_t) == [seed, off]


@pytest.mark.parametrize("state", range(len(STATES)))
@pytest.mark.parametrize("n", NS)
def test_normal_equals_mirror(lib, n, state):
    """|got - mirror| <= c 2^-23 max(r, 2^-12).  Measured on the MI355X: the largest ratio over all normal cases of this
    file (these, the advancing draws, the job launches, the engine's eps) is 1.738, at n = 2 097 157 from (0, 0, 0);
    c = 3.476, twice that (NORMAL_C)."""
    seed, off, stream = STATES[state]
    rng_t = _state(seed, off)
    buf = _float_buf(n)
    assert lib.mmvae_philox_normal(n, buf.data_ptr(), rng_t.data_ptr(), stream, 0, _s()) == 0
    want, radius = M.normal_with_radius(n, seed, off, stream)
    _assert_normal(buf, n, want, radius, f"n={n} state={state}")
    assert _read(rng_t) == [seed, off]


def test_single_fills_advance_by_their_consumption(lib):
    """advance=True: offset += (n + 3) // 4, three successive draws are the mirror's at the three offsets (the second
    and third across the carry into the high counter word); advance=False leaves the state alone."""
    seed, off, n = 99, 2 ** 32 - 300, 1023
    step = (n + 3) // 4
    rng_t = _state(seed, off)
    for i in range(3):
        buf = _mask_buf(n)
        assert lib.mmvae_philox_keep_mask(n, 0.3, buf.data_ptr(), rng_t.data_ptr(), 5, 1, _s()) == 0
        _assert_mask(buf, n, M.keep_mask(n, 0.3, seed, off + i * step, 5), f"draw {i}")
        assert _read(rng_t) == [seed, off + (i + 1) * step]
    off += 3 * step
    n2 = 34  # not a multiple of 4: the partial counter is consumed whole
    for i in range(3):
        buf = _float_buf(n2)
        assert lib.mmvae_philox_normal(n2, buf.data_ptr(), rng_t.data_ptr(), 6, 1, _s()) == 0
        want, radius = M.normal_with_radius(n2, seed, off + i * 9, 6)
        _assert_normal(buf, n2, want, radius, f"advancing draw {i}")
        assert _read(rng_t) == [seed, off + (i + 1) * 9]
    before = _read(rng_t)
    assert lib.mmvae_philox_keep_mask(n, 0.3, _mask_buf(n).data_ptr(), rng_t.data_ptr(), 5, 0, _s()) == 0
    assert lib.mmvae_philox_normal(n2, _float_buf(n2).data_ptr(), rng_t.data_ptr(), 6, 0, _s()) == 0
    assert _read(rng_t) == before


def test_philox_advance_adds_exactly(lib):
    seed = U64 - 12345
    rng_t = _state(seed, 2 ** 32 - 3)
    want = 2 ** 32 - 3
    for by in (10, 0, 1, 2 ** 40 + 1, 2 ** 63, 2 ** 63 - 2 ** 40 + 5):  # across 2^32, 2^63 and the wrap at 2^64
        assert lib.mmvae_philox_advance(rng_t.data_ptr(), by, _s()) == 0
        want = (want + by) & U64
        assert _read(rng_t) == [seed, want], by
    from mmvae_amd import _lib

    assert lib.mmvae_philox_advance(None, 1, _s()) == _lib.ERR_ARG


# ------------------------------------------------------------------------------------------------- job launches
class _Jobs:
    """Five fills of one launch: masks of 200 003, 4096 and 7 elements, normals of 150 001 and 33 (the two large ones
    beyond the 131 072 elements that 128 workgroups cover in one pass), distinct stream ids."""
    SPEC = [(0, 200003, 11, 0.1), (0, 4096, 12, 0.5), (0, 7, 2 ** 32 + 13, 0.25), (1, 150001, 21, 0.0), (1, 33, 22, 0.0)]

    def __init__(self):
        from mmvae_amd import _lib

        self.bufs = [(_mask_buf if kind == 0 else _float_buf)(n) for kind, n, _, _ in self.SPEC]
        jobs = [_lib.PhiloxJob(b.data_ptr(), n, sid, p, kind) for b, (kind, n, sid, p) in zip(self.bufs, self.SPEC)]
        arr = (_lib.PhiloxJob * len(jobs))(*jobs)
        self.dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        self.n_max = max(n for _, n, _, _ in self.SPEC)
        self.advance_by = (self.n_max + 3) // 4

    def reset(self):
        for b, (kind, _, _, _) in zip(self.bufs, self.SPEC):
            b.fill_(GUARD_BYTE if kind == 0 else GUARD_FLOAT)

    def check(self, seed, offset, what):
        for k, (b, (kind, n, sid, p)) in enumerate(zip(self.bufs, self.SPEC)):
            if kind == 0:
                _assert_mask(b, n, M.keep_mask(n, p, seed, offset, sid), f"{what} job {k}")
            else:
                want, radius = M.normal_with_radius(n, seed, offset, sid)
                _assert_normal(b, n, want, radius, f"{what} job {k}")

    def untouched(self):
        return all(bool((b == (GUARD_BYTE if kind == 0 else GUARD_FLOAT)).all())
                   for b, (kind, _, _, _) in zip(self.bufs, self.SPEC))


def test_fill_jobs_advance_eager_and_captured(lib):
    """mmvae_philox_fill_jobs_advance, the launch at the head of every production-mode program: four eager launches,
    then ONE captured launch replayed three times.  After every run each job is the mirror's fill at offset0 + i *
    advance_by, the ticket word is back at 0 and the counter has advanced exactly once (the second run starts below
    2^32 and ends above it)."""
    from mmvae_amd import _lib

    J = _Jobs()
    seed, off0 = 1234, 2 ** 32 - 70000
    rng_t = _state(seed, off0)
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")

    def launch():
        return lib.mmvae_philox_fill_jobs_advance(len(J.SPEC), J.dev.data_ptr(), J.n_max, rng_t.data_ptr(), J.advance_by,
                                                  ticket.data_ptr(), _s())

    def after(i, what):
        torch.cuda.synchronize()
        J.check(seed, off0 + i * J.advance_by, f"{what} run {i}")
        assert int(ticket[0]) == 0, f"{what} run {i}: the ticket word was left at {int(ticket[0])}"
        assert _read(rng_t) == [seed, off0 + (i + 1) * J.advance_by], f"{what} run {i}"

    for i in range(4):
        J.reset()
        assert launch() == 0
        after(i, "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):  # as PlanRun.run captures a program's segments
        rc = launch()
    assert rc == 0
    assert _read(rng_t) == [seed, off0 + 4 * J.advance_by]  # capturing draws nothing
    for i in range(4, 7):
        J.reset()
        g.replay()
        after(i, "replayed")
    g.reset()

    # argument checks: nothing is launched, nothing moves
    J.reset()
    before = _read(rng_t)
    args = (J.dev.data_ptr(), J.n_max, rng_t.data_ptr())
    assert lib.mmvae_philox_fill_jobs_advance(len(J.SPEC), *args, 0, ticket.data_ptr(), _s()) == _lib.ERR_ARG
    assert lib.mmvae_philox_fill_jobs_advance(len(J.SPEC), *args, J.advance_by, None, _s()) == _lib.ERR_ARG
    assert lib.mmvae_philox_fill_jobs_advance(0, *args, J.advance_by, ticket.data_ptr(), _s()) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert _read(rng_t) == before and int(ticket[0]) == 0 and J.untouched()


def test_fill_jobs_grid_stride_at_the_2048_workgroup_cap(lib):
    from mmvae_amd import _lib

    seed, off, stream = STATES[1]
    n = NS[-1]
    buf = _mask_buf(n)
    arr = (_lib.PhiloxJob * 1)(_lib.PhiloxJob(buf.data_ptr(), n, stream, 0.1, 0))
    jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    rng_t = _state(seed, off)
    assert lib.mmvae_philox_fill_jobs(1, jobs.data_ptr(), n, rng_t.data_ptr(), _s()) == 0
    _assert_mask(buf, n, M.keep_mask(n, 0.1, seed, off, stream), "fill_jobs")
    assert _read(rng_t) == [seed, off]


# ------------------------------------------------------------------------------------------------- the engine's draws
def _build_model(tmp_path):
    """The sizes of test_philox_production_noise_trains (tests/test_properties_gpu.py), with per-layer dropout: the expert
    encoder's FIRST layer has none (so it holds no keep mask) and its second has, the shared encoder and both decoders
    have some, and two adversaries with dropout sit on the hidden representation and on z."""
    import warnings

    import torch.nn as nn

    from mmvae_amd import synthetic
    from mmvae_amd.config import AutogradConfig, GradientClipConfig
    from mmvae_amd.models import CMMVAEModel
    from mmvae_amd.modules import CMMVAE, CLVAE, base

    def cfg(layers, **kw):
        return base.FCBlockConfig(layers=list(layers), activation_fn=kw.pop("act", nn.ReLU), **kw)

    G, Z, h1, h2, hv = 512, 16, 64, 32, 24
    classes = {"assay": 8, "sex": 2}
    torch.manual_seed(0)
    exps = [base.Expert("human", cfg([G, h1, h2], dropout_rate=[0.0, 0.2], use_batch_norm=True),
                        cfg([h2, h1, G], dropout_rate=[0.25, 0.0]))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = CLVAE(latent_dim=Z, encoder_config=cfg([h2, hv], dropout_rate=0.1, use_batch_norm=True, return_hidden=True),
                    decoder_config=cfg([Z, hv, h2], dropout_rate=[0.0, 0.15]), hidden_z=True)
    base.Adversarial.labels.clear()
    labels_dir = synthetic.write_label_dir(str(tmp_path), classes)
    advs = [base.Adversarial(cfg([hv, 32, 16], dropout_rate=[0.0, 0.3]), cfg([16], act=None), list(classes), labels_dir),
            base.Adversarial(cfg([Z, 16], dropout_rate=0.2), cfg([16], act=None), list(classes), labels_dir)]
    clip = lambda: GradientClipConfig(val=10, algorithm="norm")  # noqa: E731
    model = CMMVAEModel(CMMVAE(vae, base.Experts(exps), advs), adv_weight=1.0,
                        autograd_config=AutogradConfig(clip(), clip(), clip()), use_engine=True).cuda()
    x = synthetic.synthetic_counts(64, G, device="cuda")
    return model, x, synthetic.synthetic_metadata(64, seed=5, classes=classes)


def test_engine_production_mode_draws_the_mirrors_numbers(tmp_path):
    """Production mode (no explicit noise): after a training step every keep mask of the program is the mirror's at the
    pre-step offset on stream STREAM_DROPOUT + its id, all ids differ, eps is the mirror's normal fill on STREAM_NORMAL,
    and the counter has advanced by (n_max + 3) // 4.  Four steps on the same batch: every one at its own offset, no mask
    equal to the step's before, and at least one of them a replay of a captured program."""
    from mmvae_amd import rng

    from mmvae_amd.modules import base

    assert (rng.STREAM_DROPOUT, rng.STREAM_NORMAL) == (STREAM_DROPOUT, STREAM_NORMAL)
    labels_before = {c: dict(v) for c, v in base.Adversarial.labels.items()}  # class-level: put back for later tests
    model, x, meta = _build_model(tmp_path)
    model.train()
    model.trainer.set_stage("training")
    model.optimizers()
    st = rng.state(torch.device("cuda", 0))
    rng.reseed(4321)
    previous = None
    try:
        for step in range(4):
            seed, off = _read(st)
            model.training_step((x, meta, "human"), step)
            model._flush_engine()
            torch.cuda.synchronize()
            assert model._engine, "the engine declined the model"
            plan = model._engine.last_plan
            assert not plan.explicit and plan.n_adv == 2
            layers = list(plan._mask_layers)
            ids = [sid for _, sid in layers]
            # expert encoder layer 1, shared encoder, shared decoder layer 1, expert decoder layer 0, and per phase
            # adversary 1 layer 1 and adversary 2 layer 0
            assert len(layers) == 4 + 2 * 2
            assert len(set(ids)) == len(ids), f"keep masks of one step share Philox stream ids: {sorted(ids)}"
            n_max = plan.K * plan.B * plan.Z
            for l, sid in layers:
                n = l.mask.numel()
                n_max = max(n_max, n)
                assert 0.0 < l.p < 1.0
                got = l.mask.reshape(-1).cpu().numpy()
                want = M.keep_mask(n, l.p, seed, off, STREAM_DROPOUT + sid)
                assert np.array_equal(got, want), f"step {step}: mask of stream id {sid} ({n} elements, p={l.p})"
            n = plan.eps.numel()
            assert tuple(plan.eps.shape) == (plan.K, plan.B, plan.Z)
            want, radius = M.normal_with_radius(n, seed, off, STREAM_NORMAL)
            got = plan.eps.reshape(-1).cpu().numpy()
            assert bool(np.isfinite(got).all())
            ratio = np.abs(got.astype(np.float64) - want) / (2.0 ** -23 * np.maximum(radius, 2.0 ** -12))
            print(f"philox normal engine step {step}: max ratio {float(ratio.max()):.3f}")
            assert float(ratio.max()) <= NORMAL_C
            assert _read(st) == [seed, off + (n_max + 3) // 4], f"step {step}"
            assert np.isfinite(float(model.logged["loss/training/human"]))
            masks = [l.mask.clone() for l, _ in layers]
            if previous is not None:
                assert all(a.shape == b.shape and not torch.equal(a, b) for a, b in zip(previous, masks)), f"step {step}"
            previous = masks
        eng = model._engine
        assert eng.settings.graphs and not eng.eager_only  # (then a plan's second run on is a graph replay)
        assert max(p._runs for p in eng._plans.values()) >= 2
    finally:
        if model._engine:
            model._engine.close()
        base.Adversarial.labels.clear()
        base.Adversarial.labels.update(labels_before)


# ------------------------------------------------------------------------------------------------- small neighbours
@pytest.mark.parametrize("H", [1, 4, 7])
@pytest.mark.parametrize("n", [1, 33, 4644])
def test_sum_rows(lib, H, n):
    """out_each[h] against an fp64 row sum (1e-6 of the row's sum of absolute values); out_total bitwise the float sum
    of out_each in row order; the padding between rows (ld > n) is never read; either output may be NULL."""
    from mmvae_amd import _lib

    ld = n + 5
    g = torch.Generator().manual_seed(100 * H + n)
    v = torch.randn(H, ld, generator=g)
    v[:, n:] = float("nan")
    vd = v.cuda()
    ref = v[:, :n].double().sum(1).numpy()
    mag = v[:, :n].double().abs().sum(1).numpy()

    def run(want_each, want_total):
        each = torch.full((H + 4,), GUARD_FLOAT, device="cuda")
        total = torch.full((4,), GUARD_FLOAT, device="cuda")
        rc = lib.mmvae_sum_rows_f32(H, n, vd.data_ptr(), ld, each.data_ptr() if want_each else None,
                                    total.data_ptr() if want_total else None, _s())
        assert rc == 0
        return each.cpu().numpy(), total.cpu().numpy()

    each, total = run(True, True)
    assert bool((np.abs(each[:H].astype(np.float64) - ref) <= 1e-6 * mag).all()), (each[:H], ref)
    if n == 1:
        assert each[:H].tolist() == v[:, 0].tolist()
    acc = each[0]
    for h in range(1, H):
        acc = np.float32(acc + each[h])
    assert total[0].tobytes() == np.float32(acc).tobytes()
    assert bool((each[H:] == np.float32(GUARD_FLOAT)).all()) and bool((total[1:] == np.float32(GUARD_FLOAT)).all())
    each2, total2 = run(True, False)
    assert each2.tobytes() == each.tobytes() and bool((total2 == np.float32(GUARD_FLOAT)).all())
    each3, total3 = run(False, True)
    assert total3.tobytes() == total.tobytes() and bool((each3 == np.float32(GUARD_FLOAT)).all())
    assert lib.mmvae_sum_rows_f32(H, n, vd.data_ptr(), ld, None, None, _s()) == _lib.ERR_ARG
    out = torch.zeros(H, device="cuda")
    assert lib.mmvae_sum_rows_f32(H, n, vd.data_ptr(), n - 1, out.data_ptr(), None, _s()) == _lib.ERR_ARG  # ld < n
    assert lib.mmvae_sum_rows_f32(0, n, vd.data_ptr(), ld, out.data_ptr(), None, _s()) == _lib.ERR_ARG


@pytest.mark.parametrize("n", [1, 3, 4, 1000, 1003])
def test_axpby_both_variants(n):
    """y = alpha x + beta y on views that start 0, 4, 8 and 12 bytes off a 16-byte boundary: only (n % 4 == 0, both
    aligned) takes the 16-byte kernel.  Bitwise alpha*x + beta*y of fp32 torch where the expression rounds once; with
    two products the compiler may contract one into an fma (as in test_sum_parts_batch: 1e-6).  beta == 0 never reads
    y (pre-filled with NaN); the floats around the view stay as they were."""
    from mmvae_amd import ops

    g = torch.Generator().manual_seed(n)
    for xo in range(4):
        for yo in range(4):
            for alpha, beta in ((2.5, -0.3), (2.0, -0.5), (1.0, 1.0), (-1.5, 0.0), (1.0, 0.0)):
                xb = torch.randn(n + 8, generator=g).cuda()
                yb = torch.randn(n + 8, generator=g).cuda()
                assert xb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
                if beta == 0.0:
                    yb[yo:yo + n] = float("nan")
                x, y = xb[xo:xo + n], yb[yo:yo + n]
                assert x.data_ptr() % 16 == 4 * xo and y.data_ptr() % 16 == 4 * yo
                y0 = yb.clone()
                ref = alpha * x if beta == 0.0 else alpha * x + beta * y
                out = ops.axpby(alpha, x, beta, y)
                what = (n, xo, yo, alpha, beta)
                assert out.data_ptr() == y.data_ptr()
                assert not bool(torch.isnan(y).any()), what
                if beta == 0.0 or (alpha, beta) in ((2.0, -0.5), (1.0, 1.0)):  # exact products: one rounding
                    assert torch.equal(y, ref), what
                else:
                    assert torch.allclose(y, ref, rtol=1e-6, atol=1e-6), what
                assert torch.equal(yb[:yo], y0[:yo]) and torch.equal(yb[yo + n:], y0[yo + n:]), what
