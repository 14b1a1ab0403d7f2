"""The meta-discriminators on the GPU: the fused kernel of libmmvae_disc.so against its fp64 definition
(functional.meta_disc_tail on CPU plumbing), its reproducibility and its summation order, MetaDiscriminator.train_step
against fp64 nn.Sequential + torch.optim.Adam, and MetaDiscriminators.step through the captured cross-generation program
against the CPU-plumbing run of the same model.

Kernel tolerance: per shape, the error of the SAME function evaluated by stock torch in fp32 on the CPU (autograd of
sigmoid / F.binary_cross_entropy) against the fp64 definition -- the largest, over the eight results, of max |error| /
max |reference| -- is the yardstick; the kernel is allowed 4 x that on every result, for its different summation order.
Both figures are printed per shape (DESIGN.md records them)."""
import functools

import pandas as pd
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402

SHAPES = [(1, 1, 1), (15, 5, 3), (17, 128, 64), (130, 256, 64), (512, 128, 64), (513, 128, 128)]
RESULTS = ("p", "loss", "dpre1", "db1", "dW2", "db2", "dW3", "db3")
GUARD = 64
SENTINEL = -777.0


def _inputs(B, H1, H2, seed=None):
    """fp32 inputs with every hidden sigmoid inside (1e-4, 1 - 1e-4) (|pre-activation| < 9.2) and |s| <= 25; mixed labels."""
    g = torch.Generator().manual_seed(1000 * B + H1 + H2 if seed is None else seed)
    pre1 = (1.5 * torch.randn(B, H1, generator=g)).clamp(-6.0, 6.0)
    W2 = torch.randn(H2, H1, generator=g) * (2.0 / H1 ** 0.5)
    b2 = 0.5 * torch.randn(H2, generator=g)
    W3 = torch.randn(1, H2, generator=g) * (3.0 / H2 ** 0.5)
    b3 = 0.3 * torch.randn(1, generator=g)
    y = (torch.rand(B, generator=g) > 0.5).float()
    if B > 4:
        y[3] = 0.25  # one soft label
    a2 = torch.sigmoid(pre1.double()) @ W2.double().T + b2.double()
    s = torch.sigmoid(a2) @ W3.double().reshape(-1) + b3.double()
    assert float(pre1.abs().max()) <= 6.0 and float(a2.abs().max()) < 9.2 and float(s.abs().max()) <= 25.0
    return pre1, W2, b2, W3, b3, y


def _flat(p, out, dpre1, grads):
    return dict(zip(RESULTS, (p, out[0], dpre1) + tuple(grads))), float(out[1])


@functools.lru_cache(maxsize=None)
def _reference(B, H1, H2):
    """(inputs, fp64 definition, hit fraction, yardstick): computed once per shape and shared."""
    from mmvae_amd import backend
    from mmvae_amd import functional as HF

    inp = _inputs(B, H1, H2)
    with backend.cpu_plumbing():
        want, hits = _flat(*HF.meta_disc_tail(*inp, train=True))
    # stock torch in fp32 on the CPU
    pre1, W2, b2, W3, b3, y = (t.clone() for t in inp)
    for t in (pre1, W2, b2, W3, b3):
        t.requires_grad_(True)
    p = torch.sigmoid(torch.sigmoid(torch.sigmoid(pre1) @ W2.T + b2) @ W3.T + b3)
    loss = F.binary_cross_entropy(p, y[:, None], reduction="mean")
    loss.backward()
    stock = dict(zip(RESULTS, (p.detach().flatten(), loss.detach(), pre1.grad, pre1.grad.sum(0), W2.grad, b2.grad, W3.grad,
                               b3.grad)))
    yardstick = max(_err(stock[k], want[k]) for k in RESULTS)
    return inp, want, hits, yardstick


def _err(got, want):
    got, want = got.detach().double().cpu().flatten(), want.detach().double().cpu().flatten()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _guarded(*shape, device="cuda"):
    """A contiguous tensor of this shape inside a sentinel-filled buffer, GUARD floats on either side."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _call(inp, train=True, pad=3, guarded=False):
    """ops.disc_tail on the device with ld1 = ldd = H1 + pad; returns the results and the raw buffers."""
    from mmvae_amd import ops

    pre1, W2, b2, W3, b3, y = (t.cuda() for t in inp)
    B, H1 = pre1.shape
    H2 = b2.numel()
    wide = torch.full((B, H1 + pad), 55.0, dtype=torch.float32, device="cuda")
    wide[:, :H1] = pre1
    bufs = {}
    kw = {}
    if guarded:
        bufs["out"], kw["out"] = _guarded(2)
        if train:
            bufs["dpre1"], dwide = _guarded(B, H1 + pad)
            kw["dpre1"] = dwide[:, :H1]
            names = ("db1", "dW2", "db2", "dW3", "db3")
            shapes = ((H1,), (H2, H1), (H2,), (1, H2), (1,))
            views = []
            for n_, s_ in zip(names, shapes):
                bufs[n_], v = _guarded(*s_)
                views.append(v)
            kw["grads"] = tuple(views)
    elif train:
        kw["dpre1"] = torch.empty((B, H1 + pad), dtype=torch.float32, device="cuda")[:, :H1]
    res = ops.disc_tail(wide[:, :H1], W2, b2, W3, b3, y, train=train, **kw)
    torch.cuda.synchronize()
    return res, bufs


@pytest.mark.parametrize("B,H1,H2", SHAPES)
def test_kernel_against_the_fp64_definition(B, H1, H2):
    inp, want, hits, yardstick = _reference(B, H1, H2)
    (p, out, dpre1, grads), bufs = _call(inp, train=True, guarded=True)
    got, got_hits = _flat(p, out, dpre1, grads)
    errs = {k: _err(got[k], want[k]) for k in RESULTS}
    worst = max(errs.values())
    print(f"disc_tail ({B}, {H1}, {H2}): stock fp32 torch {yardstick:.3g}, kernel {worst:.3g} "
          f"({', '.join(f'{k} {v:.2g}' for k, v in errs.items())})")
    # guard floats on either side of every output, and the pad columns of dpre1
    for name, buf in bufs.items():
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), name
    dwide = bufs["dpre1"][GUARD:-GUARD].view(B, H1 + 3)
    assert bool((dwide[:, H1:] == SENTINEL).all())
    assert bool(torch.isfinite(dpre1).all()) and p.shape == (B,) and dpre1.shape == (B, H1)
    assert abs(got_hits - hits) <= 2.0 ** -23  # (the fraction is rounded to fp32)
    for k in RESULTS:
        assert errs[k] <= 4.0 * yardstick, (k, errs[k], yardstick)


@pytest.mark.parametrize("B,H1,H2", [(130, 256, 64), (513, 128, 128)])
def test_reproducible_and_forward_only_bits(B, H1, H2):
    inp = _reference(B, H1, H2)[0]
    (p1, out1, d1, g1), _ = _call(inp, train=True)
    (p2, out2, d2, g2), _ = _call(inp, train=True)
    assert torch.equal(p1, p2) and torch.equal(out1, out2) and torch.equal(d1, d2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    (pf, outf, df, gf), bufs = _call(inp, train=False, guarded=True)
    assert df is None and gf is None
    assert torch.equal(pf, p1) and torch.equal(outf, out1)
    assert bool((bufs["out"][:GUARD] == SENTINEL).all()) and bool((bufs["out"][-GUARD:] == SENTINEL).all())
    # no labels: p alone
    from mmvae_amd import ops

    pre1, W2, b2, W3, b3, _ = (t.cuda() for t in inp)
    p_only, none_out, _, _ = ops.disc_tail(pre1, W2, b2, W3, b3)
    assert none_out is None and torch.equal(p_only, p1)


def test_tile_loop_adds_the_tiles_in_order():
    """B = 4096 is 256 tiles of 16 rows on a grid capped at 128 workgroups: every workgroup loops.  The definition of the
    order: a tile's partial adds its rows in row order, the partials are added in tile order, starting from zero.  A call
    on one tile alone (B = 16) returns that tile's partial, scaled by 4096 / 16 = 2^8 -- exactly, the 1 / B being a power
    of two in both calls -- so the 256 single-tile calls, rescaled and added up in fp32 in tile order on the host, must
    give the bits of the one call."""
    from mmvae_amd import _disc_lib

    B, H1, H2 = 4096, 128, 64
    rows = _disc_lib.DISC_TILE_ROWS
    assert B // rows > _disc_lib.DISC_GRID_CAP
    inp = _inputs(B, H1, H2)
    (p, out, dpre1, grads), _ = _call(inp, train=True, pad=0)
    scale = rows / B
    acc = [torch.zeros_like(g, device="cpu") for g in grads]
    loss = torch.zeros((), dtype=torch.float32)
    hits = 0.0
    pre1, W2, b2, W3, b3, y = inp
    for t in range(B // rows):
        sl = slice(t * rows, (t + 1) * rows)
        (pt, outt, dt, gt), _ = _call((pre1[sl], W2, b2, W3, b3, y[sl]), train=True, pad=0)
        assert torch.equal(pt, p[sl]) and torch.equal(dt * scale, dpre1[sl]), t
        for a, g in zip(acc, gt):
            a += g.cpu() * scale
        loss += outt[0].cpu() * rows
        hits += float(outt[1]) * rows
    for name, a, g in zip(RESULTS[3:], acc, grads):
        assert torch.equal(a, g.cpu()), name
    assert float(loss / B) == float(out[0]) and hits / B == float(out[1])


def _fp64_twin(disc):
    seq = disc.as_sequential().double()
    return seq, torch.optim.Adam(seq.parameters(), lr=1e-3)


@pytest.mark.parametrize("in_features,B", [(257, 33), (128, 512)])
def test_three_train_steps_against_fp64_torch(in_features, B):
    """Losses: the fp32 forward is three dot products of length in, H1 and H2 and a mean, (in + H1 + H2 + 16) 2^-24
    relative in the worst case.  Parameters after Adam: rel-L2 <= 1e-4, the project's bound."""
    from mmvae_amd.modules.meta_discriminator import MetaDiscriminator

    torch.manual_seed(in_features)
    disc = MetaDiscriminator(in_features)
    seq, opt = _fp64_twin(disc)
    disc = disc.cuda()
    g = torch.Generator().manual_seed(B)
    loss_tol = (in_features + 128 + 64 + 16) * 2.0 ** -24
    for step in range(3):
        x = torch.relu(torch.randn(B, in_features, generator=g))
        y = (torch.rand(B, generator=g) > 0.5).float() if step != 1 else 1.0  # a tensor of labels, or one for all rows
        loss, acc = disc.train_step(x.cuda(), y.cuda() if isinstance(y, torch.Tensor) else y)
        opt.zero_grad()
        yt = y.double() if isinstance(y, torch.Tensor) else torch.full((B,), y, dtype=torch.float64)
        p = seq(x.double())
        want = F.binary_cross_entropy(p, yt[:, None], reduction="mean")
        want.backward()
        opt.step()
        want_acc = float(((p.detach().flatten() > 0.5) == (yt > 0.5)).double().mean())
        print(f"in {in_features} B {B} step {step}: loss {float(loss):.8f} against {float(want):.8f}")
        assert abs(float(loss) - float(want)) <= loss_tol * float(want), step
        assert abs(float(acc) - want_acc) <= 1.0 / B + 1e-6, step  # (a row within rounding of p = 0.5 may fall either way)
    for (name, got), want in zip(disc.state_dict().items(), seq.state_dict().values()):
        err = H.rel_l2(got, want)
        print(f"in {in_features} B {B}: {name} rel-L2 {err:.3g}")
        assert err <= 1e-4, (name, err)
    x = torch.relu(torch.randn(B, in_features, generator=g))
    p_dev = disc(x.cuda())
    assert p_dev.shape == (B, 1)
    assert float((p_dev.cpu().double() - seq(x.double()).detach()).abs().max()) <= 1e-4 + loss_tol


def _model(experts, tmpdir, device):
    from tests import mirror_utils as MU

    case = {"seed": 5, "experts": experts, "expert_hidden": [48, 24], "vae_hidden": [16], "Z": 10, "B": 33, "dropout": 0.0,
            "hidden_z": False}
    torch.manual_seed(case["seed"])
    model = MU.build_mirror(case, device, tmpdir, use_engine=True)
    model.eval()
    model.trainer.set_stage("prediction")
    return model


def test_step_end_to_end_against_cpu_plumbing(tmp_path):
    """MetaDiscriminators.step on a two-expert model with odd gene counts through the captured cross-generation program
    against the CPU-plumbing run of the same model, discriminators and batches.  The generations agree to rel-L2 2e-5
    (tests/test_crossgen_gpu.py); losses and post-Adam parameters are held to 1e-4."""
    from mmvae_amd import backend
    from mmvae_amd.modules.meta_discriminator import MetaDiscriminators

    experts, B = {"human": 257, "mouse": 130}, 33
    g = torch.Generator().manual_seed(2)
    eps = torch.randn(B, 10, generator=g)
    batches = []
    for eid in ("human", "mouse", "mouse", "human"):
        batches.append((torch.relu(torch.randn(B, experts[eid], generator=g)), eid))
    with backend.cpu_plumbing():
        cpu_model = _model(experts, str(tmp_path / "cpu"), "cpu")
        cpu_model.module.vae.encoder.explicit_eps = eps
        torch.manual_seed(9)
        cpu_mds = MetaDiscriminators(cpu_model)
        start = {k: v.clone() for k, v in cpu_mds.state_dict().items()}
        cpu_mds.trace = []
        cpu_losses = [cpu_mds.step((x, pd.DataFrame({"dummy": [0] * B}), eid)) for x, eid in batches]
    model = _model(experts, str(tmp_path / "gpu"), "cuda")
    model.module.load_state_dict({k: v.clone() for k, v in cpu_model.module.state_dict().items()})
    model.module.vae.encoder.explicit_eps = eps.cuda()
    mds = MetaDiscriminators(model)
    mds.load_state_dict(start)
    assert next(mds.parameters()).is_cuda
    mds.trace = []
    losses = [mds.step((x.cuda(), pd.DataFrame({"dummy": [0] * B}), eid)) for x, eid in batches]
    torch.cuda.synchronize()
    assert model._engine and model._engine.last_forward_key[0] == "generate"  # the captured program ran
    assert mds.trace == cpu_mds.trace
    assert mds.trace[:2] == [("latent", "z", 0.0), ("mouse", "xhat_mouse", 0.0)]
    for i, (got, want) in enumerate(zip(losses, cpu_losses)):
        assert list(got) == list(want) == ["latent", batches[i][1]]
        for k in want:
            print(f"batch {i} {k}: {float(got[k]):.8f} against {float(want[k]):.8f}")
            assert got[k].is_cuda and abs(float(got[k]) - float(want[k])) <= 1e-4 * float(want[k]), (i, k)
    want_sd = cpu_mds.state_dict()
    for name, got in mds.state_dict().items():
        err = H.rel_l2(got, want_sd[name])
        assert err <= 1e-4, (name, err)
        assert H.rel_l2(got, start[name]) > 1e-4, name  # (trained)
