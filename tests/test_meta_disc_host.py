"""Host-side checks of the meta-discriminators (no GPU): the C-ABI surface of libmmvae_disc.so and its argument
validation, the fp64 definition (functional.meta_disc_tail) against autograd of the reference's nn.Sequential under
F.binary_cross_entropy, the saturated tails, state_dict exchange with nn.Sequential, and the training policy of
runners/meta_discriminators.py restated with stock torch against train_meta_discriminators on CPU plumbing."""
import os
import re

import pandas as pd
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_disc.h")
NAMES = {"mmvae_disc_abi_version", "mmvae_disc_build_arch", "mmvae_disc_tail_workspace_bytes", "mmvae_disc_tail_f32"}


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _disc_lib

    header = open(HEADER).read()
    declared = check_surface(_disc_lib.BINDING)
    assert set(declared) == NAMES == set(_disc_lib.DISC_PROTOTYPES)
    assert declared["mmvae_disc_tail_f32"] == 22
    for word in ("MAX_H1", "MAX_H2", "MAX_W2", "TILE_ROWS", "GRID_CAP"):
        value = int(re.search(r"#define\s+MMVAE_DISC_" + word + r"\s+(\d+)", header).group(1))
        assert value == getattr(_disc_lib, "DISC_" + word), word


def test_versions_and_arch():
    from mmvae_amd import _disc_lib, _lib, _stats_lib

    header = open(HEADER).read()
    assert int(re.search(r"#define\s+MMVAE_DISC_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    lib = _disc_lib.load_disc()
    assert lib.mmvae_disc_abi_version() == 1 == _disc_lib.DISC_ABI_VERSION
    assert lib.mmvae_disc_build_arch() == b"gfx950"
    # the two other libraries are untouched: same versions, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    assert _stats_lib.load_stats().mmvae_stats_abi_version() == 1
    assert not [n for n in list(_lib.PROTOTYPES) + list(_stats_lib.STATS_PROTOTYPES) if n.startswith("mmvae_disc_")]
    assert not hasattr(_lib.load(), "mmvae_disc_tail_f32") and not hasattr(_stats_lib.load_stats(), "mmvae_disc_tail_f32")


def test_refused_shapes_launch_nothing():
    """Every refusal comes back from the host-side validation, ahead of any launch: the pointers below are never
    dereferenced (there is no device here), they only have to be non-null and aligned."""
    from mmvae_amd import _disc_lib
    from mmvae_amd._lib import ERR_ARG

    lib = _disc_lib.load_disc()
    need = lib.mmvae_disc_tail_workspace_bytes
    assert need(512, 128, 64) == 32 * ((128 * 64 + 2 * 64 + 128 + 3 + 3) // 4 * 4) * 4
    assert need(1, 1, 1) > 0 and need(1, 1, 1) % 8 == 0 and need(513, 128, 128) % 8 == 0
    assert need(16, 128, 64) == need(1, 128, 64) and need(17, 128, 64) == 2 * need(16, 128, 64)
    for shape in ((0, 128, 64), (8, 257, 8), (8, 0, 8), (8, 8, 0), (8, 8, 129), (8, 256, 65), (8, 129, 128), (-3, 8, 8)):
        assert need(*shape) == 0, shape

    P = 0x10000  # a non-null, 16-byte aligned address

    def call(B=8, H1=128, H2=64, ld1=None, ldd=None, y=P, p=P, out=P, dpre1=P, grads=(P,) * 5, ws=P, ws_bytes=None):
        ld1 = H1 if ld1 is None else ld1
        ldd = H1 if ldd is None else ldd
        ws_bytes = need(B, H1, H2) if ws_bytes is None else ws_bytes
        return lib.mmvae_disc_tail_f32(B, H1, H2, P, ld1, P, P, P, P, y, p, out, dpre1, ldd, *grads, ws, ws_bytes, None)

    assert call(H1=257, H2=8, ws_bytes=1 << 30) == ERR_ARG
    assert call(H1=256, H2=65, ws_bytes=1 << 30) == ERR_ARG  # H1 * H2 > 16384
    assert call(H2=129, ws_bytes=1 << 30) == ERR_ARG
    assert call(B=0, ws_bytes=1 << 30) == ERR_ARG
    assert call(ld1=127) == ERR_ARG
    assert call(ldd=127) == ERR_ARG
    for i in range(5):  # a gradient pointer without dpre1
        assert call(dpre1=None, grads=tuple(P if j == i else None for j in range(5))) == ERR_ARG, i
        assert call(grads=tuple(None if j == i else P for j in range(5))) == ERR_ARG, i  # ... and dpre1 without one
    assert call(y=None) == ERR_ARG  # training needs labels
    assert call(y=None, dpre1=None, grads=(None,) * 5) == ERR_ARG  # out without labels
    assert call(y=None, dpre1=None, grads=(None,) * 5, out=None, p=None) == ERR_ARG  # nothing to compute
    assert call(ws_bytes=need(8, 128, 64) - 4) == ERR_ARG  # short workspace
    assert call(ws=None) == ERR_ARG
    assert call(ws=P + 4) == ERR_ARG  # misaligned workspace


def _sequential(in_features, H1, H2):
    return nn.Sequential(nn.Linear(in_features, H1), nn.Sigmoid(), nn.Linear(H1, H2), nn.Sigmoid(), nn.Linear(H2, 1),
                         nn.Sigmoid())


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("B,H1,H2", [(1, 5, 3), (33, 128, 64), (130, 256, 64)])
def test_definition_against_autograd(B, H1, H2):
    from mmvae_amd import backend
    from mmvae_amd import functional as HF

    torch.manual_seed(B + H1)
    seq = _sequential(7, H1, H2).double()
    x = torch.randn(B, 7, dtype=torch.float64)
    y = torch.rand(B, dtype=torch.float64).round()
    if B > 2:
        y[0], y[1], y[2] = 0.0, 1.0, 0.3  # mixed labels, one of them soft
    pre1 = (x @ seq[0].weight.T + seq[0].bias).detach().requires_grad_(True)
    p_ref = seq[5](seq[4](seq[3](seq[2](seq[1](pre1)))))
    loss = F.binary_cross_entropy(p_ref, y[:, None], reduction="mean")
    loss.backward()
    with backend.cpu_plumbing():
        p, out, dpre1, grads = HF.meta_disc_tail(pre1.detach(), seq[2].weight.data, seq[2].bias.data, seq[4].weight.data,
                                                 seq[4].bias.data, y, train=True)
        p_f, out_f, none_d, none_g = HF.meta_disc_tail(pre1.detach(), seq[2].weight.data, seq[2].bias.data,
                                                       seq[4].weight.data, seq[4].bias.data, y)
        p_only = HF.meta_disc_tail(pre1.detach(), seq[2].weight.data, seq[2].bias.data, seq[4].weight.data, seq[4].bias.data)
    assert p.dtype == torch.float64 and p.shape == (B,) and out.shape == (2,)
    assert torch.equal(p_f, p) and torch.equal(out_f, out) and none_d is None and none_g is None
    assert torch.equal(p_only[0], p) and p_only[1] is None
    tol = 1e-12
    assert _rel(p, p_ref.detach()) <= tol
    assert abs(float(out[0]) - float(loss.detach())) <= tol * abs(float(loss.detach()))
    assert float(out[1]) == float(((p_ref.detach().flatten() > 0.5) == (y > 0.5)).double().mean())
    assert _rel(dpre1, pre1.grad) <= tol
    # db1 is the column sum of dpre1: with x constant, autograd's bias gradient of the first layer
    want = (pre1.grad.sum(0), seq[2].weight.grad, seq[2].bias.grad, seq[4].weight.grad, seq[4].bias.grad)
    for name, g, w in zip(("db1", "dW2", "db2", "dW3", "db3"), grads, want):
        assert g.shape == w.shape, name
        assert _rel(g, w) <= tol, (name, _rel(g, w))


def test_saturated_tails():
    """s = +-20 against both labels, one row at a time.  The loss is softplus(-+s), which is what torch's fp64
    -log(p) / -log(1 - p) gives up to ITS cancellation in 1 - p: an absolute error of the rounding of p near 1, 2^-53,
    over 1 - p = sigmoid(-20) = 2.06e-9, i.e. 5.4e-8 relative in 1 - p and as much absolute in its logarithm; elsewhere
    the rounding of p itself (2^-52 absolute in -log p) or 1e-12 relative.  The gradient is p - y, torch's too in fp64 (p (1 - p) = 2e-9 is above its 1e-12 clamp)."""
    import math

    from mmvae_amd import backend
    from mmvae_amd import functional as HF

    H1, H2 = 4, 2
    W2, b2 = torch.zeros(H2, H1, dtype=torch.float64), torch.zeros(H2, dtype=torch.float64)
    W3 = torch.zeros(1, H2, dtype=torch.float64)
    pre1 = torch.zeros(1, H1, dtype=torch.float64)
    tiny = 1.0 / (1.0 + math.exp(20.0))  # sigmoid(-20)
    for s in (20.0, -20.0):
        for yv in (0.0, 1.0):
            y = torch.tensor([yv], dtype=torch.float64)
            b3 = torch.tensor([s], dtype=torch.float64)  # h2 . W3 = 0: the logit is b3
            with backend.cpu_plumbing():
                p, out, dpre1, grads = HF.meta_disc_tail(pre1, W2, b2, W3, b3, y, train=True)
                _, _, _, g32 = HF.meta_disc_tail(pre1.float(), W2.float(), b2.float(), W3.float(), b3.float(), y.float(),
                                                 train=True)
            sv = torch.tensor([s], dtype=torch.float64, requires_grad=True)
            loss = F.binary_cross_entropy(torch.sigmoid(sv), y, reduction="mean")
            loss.backward()
            exact = math.log1p(math.exp(-20.0)) + (20.0 if (s > 0) == (yv == 0.0) else 0.0)  # softplus(s) or softplus(-s)
            assert abs(float(out[0]) - exact) <= 1e-14 * max(exact, 1e-9), (s, yv)
            cancelling = (s > 0) == (yv == 0.0)  # torch takes log(1 - p) with p next to 1 here
            bound = 2.0 ** -53 / tiny if cancelling else 2.0 ** -52 + 1e-12 * exact  # (-log p with p rounded next to 1)
            assert abs(float(out[0]) - float(loss.detach())) <= bound, (s, yv)
            # the gradient of the logit: p - y, in the tail that cancels -sigmoid(-s) or sigmoid(-|s|) itself
            want = (1.0 - tiny if s > 0 else tiny) - yv
            if abs(want) < 1e-6:
                want = -tiny if yv == 1.0 else tiny
            assert abs(float(grads[4]) - want) <= 1e-12 * abs(want), (s, yv)
            assert abs(float(grads[4]) - float(sv.grad)) <= max(2.0 ** -53, 1e-12 * abs(want)), (s, yv)
            assert float(p) == float(torch.sigmoid(sv.detach())) and float(out[1]) == float((s > 0) == (yv > 0.5))
            # fp32 storage changes nothing, the definition computes in fp64 (in fp32 arithmetic sigmoid(20) is exactly 1 and
            # torch's gradient exactly 0 there)
            assert float(g32[4]) == float(grads[4])
            assert float(dpre1.abs().max()) == 0.0


def test_state_dicts_load_both_ways():
    from mmvae_amd.modules.meta_discriminator import MetaDiscriminator

    torch.manual_seed(3)
    disc = MetaDiscriminator(11, hidden=(6, 5))
    seq = _sequential(11, 6, 5)
    assert list(disc.state_dict()) == list(seq.state_dict()) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
    x = torch.randn(4, 11)
    from mmvae_amd import backend

    seq.load_state_dict(disc.state_dict(), strict=True)
    with backend.cpu_plumbing():
        assert torch.equal(disc(x), seq(x)) and disc(x).shape == (4, 1)
    other = _sequential(11, 6, 5)
    disc.load_state_dict(other.state_dict(), strict=True)
    with backend.cpu_plumbing():
        assert torch.equal(disc(x), other(x))
    assert all(torch.equal(a, b) for a, b in zip(disc.as_sequential().state_dict().values(), other.state_dict().values()))
    # torch-default Linear initialisation: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weights and biases
    big = MetaDiscriminator(400, hidden=(128, 64))
    for lin in big.layers():
        bound = lin.in_features ** -0.5
        assert float(lin.weight.detach().abs().max()) <= bound and float(lin.bias.detach().abs().max()) <= bound
        assert float(lin.weight.detach().abs().max()) > 0.9 * bound
    with pytest.raises(ValueError):
        MetaDiscriminator(10, hidden=(257, 8))
    with pytest.raises(ValueError):
        MetaDiscriminator(10, hidden=(256, 65))
    with pytest.raises(RuntimeError, match="cpu_plumbing"):
        disc(x)  # a CPU tensor outside CPU plumbing is refused, as everywhere


def _tiny_model(experts: dict, tmpdir: str, device: str = "cpu"):
    from tests import mirror_utils as MU

    case = {"seed": 5, "experts": experts, "expert_hidden": [24, 12], "vae_hidden": [10], "Z": 6, "B": 9, "dropout": 0.0,
            "hidden_z": False}
    torch.manual_seed(case["seed"])
    model = MU.build_mirror(case, device, tmpdir, use_engine=True)
    model.eval()
    return model


def _batches(experts: dict, schedule, B: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for eid in schedule:
        x = torch.relu(torch.randn(B, experts[eid], generator=g))
        out.append((x, pd.DataFrame({"dummy": [0] * B}), eid))
    return out


def _reference_loop(model, batches, start: dict, labels: dict, num_epochs: int, include_cis: bool):
    """train_md (runners/meta_discriminators.py:92-167) restated with stock torch: nn.Sequential, F.binary_cross_entropy
    and torch.optim.Adam(lr=1e-3); the species branch written for any number of experts (every OTHER expert's
    discriminator on its cross generation with the source's label; the logged number is their mean)."""
    experts = list(labels)
    d = {}
    for name, sd in start.items():
        H1, in_f = sd["0.weight"].shape
        d[name] = _sequential(in_f, H1, sd["2.weight"].shape[0])
        d[name].load_state_dict(sd)
    opts = {k: torch.optim.Adam(v.parameters(), lr=1e-3) for k, v in d.items()}
    seen, history = [], []
    for _ in range(num_epochs):
        sums = {k: 0.0 for k in ["latent"] + experts}
        n = 0
        for x, metadata, eid in batches:
            n += 1
            with torch.no_grad():
                _, _, z, xhats, _ = model.module(x, metadata, eid, cross_generate=True)
            for disc in d.values():
                disc.zero_grad()
            truth = torch.full((x.shape[0], 1), labels[eid])
            loss = F.binary_cross_entropy(d["latent"](z), truth, reduction="mean")
            loss.backward()
            opts["latent"].step()
            seen.append(("latent", "z", labels[eid]))
            sums["latent"] += float(loss.detach())
            per_target = []
            for t in experts:
                if t == eid and not include_cis:
                    continue
                loss = F.binary_cross_entropy(d[t](xhats[t]), truth, reduction="mean")
                loss.backward()
                opts[t].step()
                seen.append((t, f"xhat_{t}", labels[eid]))
                per_target.append(float(loss.detach()))
            sums[eid] += sum(per_target) / len(per_target)
        history.append({f"meta_disc/md_{k}": v / n for k, v in sums.items()})
    return d, seen, history


@pytest.mark.parametrize("experts,include_cis", [({"human": 37, "mouse": 21}, False), ({"human": 37, "mouse": 21}, True),
                                                 ({"human": 19, "mouse": 21, "rat": 14}, False)])
def test_policy_on_cpu_plumbing(experts, include_cis, tmp_path):
    from mmvae_amd import backend
    from mmvae_amd.modules.meta_discriminator import MetaDiscriminators
    from mmvae_amd.trainer import Trainer
    from tests import helpers as H

    names = list(experts)
    schedule = [names[i % len(names)] for i in (0, 1, 2, 0)] if len(names) == 3 else ["human", "mouse", "mouse", "human"]
    B, hidden = 9, (16, 8)
    with backend.cpu_plumbing():
        model = _tiny_model(experts, str(tmp_path))
        model.module.vae.encoder.explicit_eps = torch.randn(B, 6, generator=torch.Generator().manual_seed(1))
        batches = _batches(experts, schedule, B)
        torch.manual_seed(17)
        mds = MetaDiscriminators(model, hidden=hidden, include_cis=include_cis)
        assert list(mds.discriminators) == ["latent"] + names
        assert mds["latent"].in_features == 6 and [mds[e].in_features for e in names] == list(experts.values())
        assert mds.labels == {e: (0.0 if i == 0 else 1.0) for i, e in enumerate(names)}
        start = {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in mds.discriminators.items()}
        mds.trace = []
        history = Trainer().meta_discriminators(model, batches, num_epochs=2, discriminators=mds)
        assert not model.module.training
        want_d, want_seen, want_history = _reference_loop(model, batches, start, mds.labels, 2, include_cis)
    assert mds.trace == want_seen
    if len(names) == 2 and not include_cis:  # the reference as written: human -> mouse's discriminator with label 0, ...
        assert mds.trace[:4] == [("latent", "z", 0.0), ("mouse", "xhat_mouse", 0.0), ("latent", "z", 1.0), ("human", "xhat_human", 1.0)]
    assert len(history) == 2 and all(list(h) == [f"meta_disc/md_{k}" for k in ["latent"] + names] for h in history)
    for got, want in zip(history, want_history):
        for k in want:
            print(k, got[k], want[k])
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), k
    for name, disc in mds.discriminators.items():
        for pname, p in disc.state_dict().items():
            err = H.rel_l2(p, want_d[name].state_dict()[pname])
            assert err <= 1e-4, (name, pname, err)
        moved = H.rel_l2(disc.state_dict()["0.weight"], start[name]["0.weight"])
        assert moved > 1e-3, name  # (the parameters really were trained)


def test_default_labels_and_unknown_source(tmp_path):
    from mmvae_amd import backend
    from mmvae_amd.modules.meta_discriminator import MetaDiscriminators, train_meta_discriminators

    with backend.cpu_plumbing():
        model = _tiny_model({"human": 13, "mouse": 11}, str(tmp_path))
        mds = MetaDiscriminators(model, hidden=(8, 4), labels={"human": 1.0, "mouse": 0.0})
        assert mds.labels == {"human": 1.0, "mouse": 0.0} and mds.targets_of("human") == ["mouse"]
        with pytest.raises(ValueError):
            MetaDiscriminators(model, labels={"human": 0.0})
        with pytest.raises(KeyError):
            mds.step((torch.zeros(2, 13), pd.DataFrame({"dummy": [0, 0]}), "rat"))
        # batches given as a callable: called once per epoch; the division is by ALL batches of the epoch
        calls = []

        def epoch():
            calls.append(1)
            return _batches({"human": 13, "mouse": 11}, ["human", "human", "mouse"], 5)

        history = train_meta_discriminators(model, epoch, num_epochs=2, hidden=(8, 4))
        assert len(calls) == 2 and len(history) == 2
        # one mouse batch in three: md_mouse is that batch's loss / 3 -- about ln 2 / 3 for a fresh discriminator, never a full loss
        assert 0.05 < history[0]["meta_disc/md_mouse"] < 0.6 and 0.1 < history[0]["meta_disc/md_human"] < 1.2
