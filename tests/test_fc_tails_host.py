"""The restatement of the layer tails (tests/fc_tail_restatement.py) and the cases of tests/test_fc_tails_gpu.py, checked
without a GPU.

1. In float64 the restatement equals torch fp64 autograd of the module order Linear output -> [BatchNorm1d(momentum 0.01,
   eps 1e-3)] -> [ReLU] -> [Dropout with an explicit mask] and of LayerNorm(no affine), running statistics and the
   addend / addend_a / row_scale gradients included, within 1e-12 of the largest reference value of each tensor, on every
   case list of the GPU file.  (The bias gradient ahead of a BatchNorm is zero in exact arithmetic: both sides are held
   to 1e-12 of the largest |dy| B instead.)
2. The two conditions the GPU tests' bounds rest on hold for the inputs alone: the restatement evaluated in float32 takes
   another ReLU slope than the float64 one on at most 0.5 % of a case's elements, and only where |y| is within the
   case's bound on y; and on the offset data float32 loses something (delta > 0) on every bounded output, except for a
   batch of one row, whose normalisation and column sums are exact (in eval mode its single element may be a ReLU zero).
"""
import numpy as np
import pytest
import torch

from tests import fc_tail_cases as FC
from tests import fc_tail_restatement as R

REL = 1e-12
FLOOR_ABS, FLOOR_REL = 1e-5, 2e-5


def close(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape
    scale = max(float(np.abs(want).max()), 1e-300) if scale is None else scale
    err = float(np.abs(got - want).max()) / scale
    assert err <= REL, err
    return err


def test_column_cases_cover_every_value_with_and_without_batchnorm():
    assert 36 <= len(FC.COLUMN_CASES) <= 48 and len(set(FC.COLUMN_CASES)) == len(FC.COLUMN_CASES)
    for bn in (True, False):
        cs = [c for c in FC.COLUMN_CASES if c.bn == bn]
        assert {c.B for c in cs} == set(FC.B_VALUES) and {c.N for c in cs} == set(FC.N_VALUES)
        assert {c.S_fwd for c in cs} == set(FC.S_VALUES) and {c.S_bwd for c in cs} == set(FC.S_VALUES)
        for opt in ("bias", "relu", "addend", "addend_a", "row_scale") + (("affine", "running", "nbt") if bn else ()):
            assert {getattr(c, opt) for c in cs} == {True, False}, (bn, opt)
        assert {c.p for c in cs} == {0.0, 0.25}
    assert {c.B for c in FC.EVAL_CASES} == {1, 9, 33, 257, 513}
    assert {c.rows for c in FC.ROW_CASES} == {1, 5, 33}
    assert {c.N for c in FC.ROW_CASES} == {1, 64, 65, 256, 512, 513, 768, 769, 1025}
    for f in ("S_fwd", "S_bwd"):
        assert {getattr(c, f) for c in FC.ROW_CASES} == {1, 3}


def _torch_column(case, inp, training):
    t = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    slabs = t(inp["slabs"]).requires_grad_(True)
    bias = t(inp["bias"]).requires_grad_(True) if case.bias else None
    z = slabs.sum(0) + (bias if bias is not None else 0.0)
    y, bn = z, None
    if case.bn:
        bn = torch.nn.BatchNorm1d(case.N, momentum=FC.MOMENTUM, eps=FC.BN_EPS, affine=case.affine,
                                  track_running_stats=case.running).double()
        if case.affine:
            bn.weight.data.copy_(t(inp["gamma"]))
            bn.bias.data.copy_(t(inp["beta"]))
        if case.running:
            bn.running_mean.copy_(t(inp["running_mean"]))
            bn.running_var.copy_(t(inp["running_var"]))
        bn.train(training)
        y = bn(z)
    a = torch.relu(y) if case.relu else y
    d = a * t(inp["mask"]) / (1.0 - case.p) if case.p > 0 else a
    return slabs, bias, bn, z, y, a, d


@pytest.mark.parametrize("data", FC.DATA)
@pytest.mark.parametrize("case", FC.COLUMN_CASES, ids=lambda c: f"{c.B}x{c.N}-{'bn' if c.bn else 'plain'}")
def test_column_restatement_equals_torch_fp64_autograd(case, data):
    inp = FC.column_inputs(case, data)
    if case.bn and case.B == 1:  # torch refuses one row under training BatchNorm: the restatement states what the entry does
        f = R.column_fwd(inp["slabs"], inp["bias"] if case.bias else None, FC.column_bn(case, inp), True, case.relu,
                         inp["mask"] if case.p > 0 else None, case.p)
        assert np.array_equal(f["mean"], f["z"][0]) and np.all(f["invstd"] == 1.0 / np.sqrt(FC.BN_EPS))
        if case.running:
            assert np.array_equal(f["running_var"], (1.0 - FC.MOMENTUM) * inp["running_var"].astype(np.float64))
        return
    t = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    slabs, bias, bn, z, y, a, d = _torch_column(case, inp, True)
    dd = t(inp["din"]).sum(0)
    if case.addend:
        dd = dd + t(inp["addend"])
    if case.row_scale:
        dd = dd * t(inp["row_scale"])[:, None]
    loss = (d * dd).sum() + ((a * t(inp["addend_a"])).sum() if case.addend_a else 0.0)
    loss.backward()
    mask, p = (inp["mask"], case.p) if case.p > 0 else (None, 0.0)
    f = R.column_fwd(inp["slabs"], inp["bias"] if case.bias else None, FC.column_bn(case, inp), True, case.relu, mask, p)
    slope = (y.detach().numpy() > 0) if case.relu else None
    b = R.column_bwd(inp["din"], f if case.bn else None, inp["gamma"] if case.bn and case.affine else None,
                     inp["addend"] if case.addend else None, inp["addend_a"] if case.addend_a else None,
                     inp["row_scale"] if case.row_scale else None, mask, p, slope)
    for k, want in (("z", z), ("y", y), ("a", a), ("d", d)):
        close(f[k], want)
    close(b["dz"], slabs.grad[0])
    for s in range(1, case.S_fwd):
        assert torch.equal(slabs.grad[s], slabs.grad[0])
    zero_scale = max(float(np.abs(b["dy"]).max()), 1e-300) * case.B
    if case.bn:
        close(f["mean"], z.detach().mean(0))
        close(f["invstd"], 1.0 / torch.sqrt(z.detach().var(0, unbiased=False) + FC.BN_EPS))
        if case.running:
            close(f["running_mean"], bn.running_mean)
            close(f["running_var"], bn.running_var)
        if case.affine:
            close(b["dgamma"], bn.weight.grad)
            close(b["dbeta"], bn.bias.grad)
        close(b["dbias"], torch.zeros(case.N, dtype=torch.float64), scale=zero_scale)
        if bias is not None:
            close(bias.grad.numpy(), torch.zeros(case.N, dtype=torch.float64), scale=zero_scale)
    else:
        if bias is not None:
            close(b["dbias"], bias.grad)
        close(b["dbias"], slabs.grad[0].sum(0))
        chunks = [slabs.grad[0][r:r + R.RPC].sum(0) for r in range(0, case.B, R.RPC)]
        close(b["partials"], torch.stack(chunks))


@pytest.mark.parametrize("data", FC.DATA)
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", FC.EVAL_CASES, ids=lambda c: f"{c.B}x{c.N}")
def test_column_restatement_in_eval_mode_equals_torch(case, with_mask, data):
    inp = FC.column_inputs(case, data)
    ev = case._replace(p=0.25 if with_mask else 0.0)
    with torch.no_grad():
        _, _, bn, z, y, a, d = _torch_column(ev, inp, False)
    f = R.column_fwd(inp["slabs"], inp["bias"] if case.bias else None, FC.column_bn(case, inp), False, case.relu,
                     inp["mask"] if with_mask else None, ev.p)
    for k, want in (("z", z), ("a", a), ("d", d)):
        close(f[k], want)
    assert f["running_mean"] is None and f["running_var"] is None and f["mean"] is None
    if data == "offset" and case.B > 1:  # float32 loses something here too
        f32 = R.column_fwd(inp["slabs"], inp["bias"] if case.bias else None, FC.column_bn(case, inp), False, case.relu,
                           inp["mask"] if with_mask else None, ev.p, np.float32)
        assert np.abs(f32["a"] - f["a"]).max() > 0 and np.abs(f32["d"] - f["d"]).max() > 0


@pytest.mark.parametrize("B,N", FC.LN_CASES)
def test_layernorm_restatement_equals_torch_fp64_autograd(B, N):
    inp = FC.ln_inputs(B, N)
    x = torch.from_numpy(np.array(inp["x"])).double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (N,), eps=FC.LN_EPS)
    g = torch.from_numpy(np.array(inp["g"])).double()
    (y * g).sum().backward()
    f = R.layernorm_fwd(inp["x"], FC.LN_EPS)
    close(f["y"], y, scale=max(float(y.detach().abs().max()), 1.0))
    close(f["mean"], x.detach().mean(1))
    close(f["invstd"], 1.0 / torch.sqrt(x.detach().var(1, unbiased=False) + FC.LN_EPS))
    close(R.layernorm_bwd(inp["g"].astype(np.float64), f["y"], f["invstd"]), x.grad,
          scale=max(float(x.grad.abs().max()), 1.0))
    if N == 1:
        assert not f["y"].any() and np.all(f["invstd"] == 1.0 / np.sqrt(FC.LN_EPS))


@pytest.mark.parametrize("case", FC.ROW_CASES, ids=lambda c: f"{c.rows}x{c.N}-{c.S_fwd}-{c.S_bwd}")
def test_rowtail_restatement_equals_torch_fp64_autograd(case):
    inp = FC.row_inputs(case)
    t = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    slabs = t(inp["slabs"]).requires_grad_(True)
    bias = t(inp["bias"]).requires_grad_(True) if case.bias else None
    v = slabs.sum(0) + (bias if bias is not None else 0.0)
    y = torch.nn.functional.layer_norm(v, (case.N,), eps=FC.LN_EPS)
    a = torch.relu(y) if case.relu else y
    d = a * t(inp["mask"]) / (1.0 - case.p) if case.p > 0 else a
    g = t(inp["din"]).sum(0)
    if case.row_scale:
        g = g * t(inp["row_scale"])[:, None]
    ((d * g).sum() + ((a * t(inp["addend"])).sum() if case.addend else 0.0)).backward()
    mask, p = (inp["mask"], case.p) if case.p > 0 else (None, 0.0)
    f = R.rowtail_fwd(inp["slabs"], inp["bias"] if case.bias else None, FC.LN_EPS, case.relu, mask, p)
    slope = (y.detach().numpy() > 0) if case.relu else None
    b = R.rowtail_bwd(inp["din"], f, inp["addend"] if case.addend else None,
                      inp["row_scale"] if case.row_scale else None, mask, p, slope)
    unit = lambda w: max(float(w.detach().abs().max()), 1.0)  # noqa: E731  (N = 1: every value is an exact zero)
    for k, want in (("y", y), ("a", a), ("d", d)):
        close(f[k], want, scale=unit(want))
    close(f["invstd"], 1.0 / torch.sqrt(v.detach().var(1, unbiased=False) + FC.LN_EPS))
    dz = slabs.grad[0]
    close(b["dz"], dz, scale=unit(dz))
    close(b["dbias"], dz.sum(0), scale=unit(dz) * case.rows)
    if bias is not None:
        close(b["dbias"], bias.grad, scale=unit(dz) * case.rows)
    close(b["partials"], torch.stack([dz[r:r + R.RPC].sum(0) for r in range(0, case.rows, R.RPC)]),
          scale=unit(dz) * R.RPC)


def test_x3_split_mirror_is_exact_and_truncating():
    rng = np.random.default_rng(3)
    v = np.float32(rng.standard_normal(4096) * np.exp2(rng.integers(-40, 40, 4096)))
    v[:3] = (0.0, -0.0, 3.0e38)
    planes = R.x3_split(v)
    assert planes.dtype == np.uint16 and planes.shape == (3, 4096)
    parts = (planes.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.array_equal((parts[0] + parts[1]) + parts[2], v)  # (as values: the sum of -0 and two +0 pieces is +0)
    assert np.array_equal(planes[0], (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16))


# --------------------------------------------------------------------------- the conditions the GPU bounds rest on
def both_dtypes(case, data):
    """(fp64, fp32) restatements of a column case, forward and backward, with the slope of the fp64 forward."""
    inp = FC.column_inputs(case, data)
    mask, p = (inp["mask"], case.p) if case.p > 0 else (None, 0.0)
    out = []
    slope = None
    for dtype in (np.float64, np.float32):
        f = R.column_fwd(inp["slabs"], inp["bias"] if case.bias else None, FC.column_bn(case, inp), True, case.relu, mask,
                         p, dtype)
        if dtype == np.float64 and case.relu:
            slope = f["y"] > 0
        b = R.column_bwd(inp["din"], f if case.bn else None, inp["gamma"] if case.bn and case.affine else None,
                         inp["addend"] if case.addend else None, inp["addend_a"] if case.addend_a else None,
                         inp["row_scale"] if case.row_scale else None, mask, p, slope, dtype)
        out.append((f, b))
    return out


def bounded_outputs(case):
    names = ["a", "d", "dz"]
    if case.bn:
        names += ["mean", "invstd"] + (["running_mean", "running_var"] if case.running else [])
        names += ["dgamma", "dbeta"]
    else:
        names += ["dbias"]
    return names


@pytest.mark.parametrize("data", FC.DATA)
@pytest.mark.parametrize("case", FC.COLUMN_CASES, ids=lambda c: f"{c.B}x{c.N}-{'bn' if c.bn else 'plain'}")
def test_float32_restatement_keeps_the_slope_and_loses_something_on_offset_data(case, data):
    (f64, b64), (f32, b32) = both_dtypes(case, data)
    assert f32["z"].dtype == np.float32 and b32["dz"].dtype == np.float32 and f32["a"].dtype == np.float32
    delta_y = float(np.abs(f32["y"].astype(np.float64) - f64["y"]).max())
    if case.relu:
        differ = (f32["y"] > 0) != (f64["y"] > 0)
        assert differ.mean() <= 0.005, differ.mean()
        assert not differ.any() or float(np.abs(f64["y"][differ]).max()) <= 4 * delta_y + FLOOR_ABS
    if data == "offset" and case.B > 1:
        for name in bounded_outputs(case):
            lo, hi = (b32, b64) if name in ("dz", "dbias", "dgamma", "dbeta") else (f32, f64)
            delta = float(np.abs(lo[name].astype(np.float64) - hi[name]).max())
            assert delta > 0, name
