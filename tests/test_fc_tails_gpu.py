"""The layer-tail kernels of mmvae_amd/csrc/fc_epilogue.hip against the fp64 restatement (tests/fc_tail_restatement.py,
itself held to torch fp64 autograd in tests/test_fc_tails_host.py): mmvae_fc_epilogue_fwd / _bwd, mmvae_layernorm_fwd /
_bwd and mmvae_fc_rowtail_fwd / _bwd, called through ctypes so that every argument is free -- leading dimensions that
differ from N, NULL options, aliasing, the workspace-only column sum, planes off a multiple of 64 columns, refusals.
The cases (tests/fc_tail_cases.py) reach one row, the 31 | 32 | 33 chunk boundary, ragged groups of eight chunk partials
(9, 10 and 17 chunks), slab counts that run the unrolled body and the remainder in one call, and the row tail's register
classes; the column tail runs on centred data and on data whose columns have a large offset.

Buffers.  Every output lies in a buffer with slack columns up to its leading dimension and sentinel rows before and
behind it, all filled with one NaN bit pattern, which must be there after every call; inputs carry the same NaN in their
slack columns, and a workspace has 8 N sentinel floats on both sides (a read beyond it poisons the result).

Bounds.  For each case and output the device's largest deviation from the fp64 restatement is at most 4 delta + floor:
delta is what the restatement itself loses on the same input when it is evaluated in float32 in the documented
summation tree, 4 covers another legitimate fp32 order (contracted multiply-adds, another tree inside a chunk), and floor
is the bound of tests/test_kernels_gpu.py::test_fc_epilogue_fwd_bwd: 1e-5 absolute for elementwise outputs and saved
statistics, 2e-5 rel-L2 for gradients.  Sums of plain additions (z, the bias gradient from its chunk partials) are
compared bit for bit.  The bias gradient ahead of a BatchNorm, zero in exact arithmetic, keeps the older rule
|dbias| <= 1e-3 max|dy| B.  The ReLU slope the device took may differ from 1[y > 0] of the fp64 restatement only where
|y| is within the case's bound on y, on at most 0.5 % of its elements.  On the offset data delta > 0 for every bounded
output (a batch of one row aside: its normalisation and column sums are exact, and in eval mode a single element under
the ReLU may be an exact zero).  Each test prints what it measured; the
largest figures per family are in profiles/fc_tails.txt.
"""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fc_tail_cases as FC
from tests import fc_tail_restatement as R

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF    # a quiet NaN with a payload no arithmetic produces
SENT16 = 0x7ABC
PAD_ROWS = 2
FLOOR_ABS, FLOOR_REL = 1e-5, 2e-5
MAXIMA = collections.defaultdict(lambda: (0.0, 0.0))  # (family, output) -> largest (deviation, its delta)

ARGS = {
    "mmvae_fc_epilogue_fwd": "B N inp ld_in n_slabs bias bn training relu keep_mask dropout_p z_out a_out d_out ld_out "
                             "save_mean save_invstd workspace workspace_bytes d_planes split stream",
    "mmvae_fc_epilogue_bwd": "B N din ld_in n_slabs addend addend_a row_scale keep_mask dropout_p relu a z gamma save_mean "
                             "save_invstd has_bn dz_out ld_out dbias dgamma dbeta workspace workspace_bytes dz_planes stream",
    "mmvae_layernorm_fwd": "B N x ldx eps y ldy save_mean save_invstd stream",
    "mmvae_layernorm_bwd": "B N dy lddy y ldy save_invstd dx lddx stream",
    "mmvae_fc_rowtail_fwd": "B N inp ld_in n_slabs bias eps training relu keep_mask dropout_p y_out a_out d_out ld_out "
                            "save_invstd stream",
    "mmvae_fc_rowtail_bwd": "B N din ld_in n_slabs addend row_scale keep_mask dropout_p relu act y save_invstd dz_out ld_out "
                            "dbias workspace workspace_bytes stream",
}


def call(name, **kw):
    """One C entry by keyword; what is not given is NULL / 0.  Buffers are passed as themselves."""
    from mmvae_amd import _lib

    lib = _lib.load()
    names, types = ARGS[name].split(), _lib.PROTOTYPES[name][1]
    assert len(names) == len(types) and not set(kw) - set(names), set(kw) - set(names)
    args = []
    for n, t in zip(names, types):
        v = kw.get(n)
        if n == "stream":
            v = torch.cuda.current_stream().cuda_stream
        elif hasattr(v, "ptr"):
            v = v.ptr()
        elif v is None and t in (C.c_int, C.c_int64, C.c_size_t):
            v = 0
        elif v is None and t is C.c_float:
            v = 0.0
        args.append(v)
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    return rc


class Mat:
    """fp32 [rows, cols] inside a sentinel-filled buffer [PAD_ROWS + rows + PAD_ROWS, ld]."""

    def __init__(self, rows, cols, ld, data=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.whole = torch.full((rows + 2 * PAD_ROWS, ld), SENT, dtype=torch.int32, device="cuda")
        self.body = self.whole[PAD_ROWS:PAD_ROWS + rows]
        if data is not None:
            self.set(data)

    def set(self, data):
        data = np.array(data, dtype=np.float32).reshape(self.rows, self.cols)  # (a copy: the cases' inputs are read-only)
        self.body[:, :self.cols] = torch.from_numpy(data.view(np.int32)).cuda()

    def ptr(self):
        return self.body.data_ptr()

    def bits(self):
        return self.body[:, :self.cols].contiguous().cpu().numpy().view(np.uint32)

    def get(self):
        return self.bits().view(np.float32)

    def slack_untouched(self):
        return bool((self.whole[:PAD_ROWS] == SENT).all() and (self.whole[PAD_ROWS + self.rows:] == SENT).all()
                    and (self.body[:, self.cols:] == SENT).all())

    def untouched(self):
        return bool((self.whole == SENT).all())


class Vec(Mat):
    """fp32 [n] with `pad` sentinel floats on both sides."""

    def __init__(self, n, data=None, pad=8):
        self.rows, self.cols, self.ld, self.pad = 1, n, n, pad
        self.whole = torch.full((n + 2 * pad,), SENT, dtype=torch.int32, device="cuda")
        self.body = self.whole[pad:pad + n].view(1, n)
        if data is not None:
            self.set(data)

    def get(self):
        return self.bits().view(np.float32)[0]

    def slack_untouched(self):
        return bool((self.whole[:self.pad] == SENT).all() and (self.whole[self.pad + self.cols:] == SENT).all())


class Slabs:
    """fp32 input slabs [S, rows, cols] with leading dimension ld (slab stride rows * ld), NaN in the slack columns."""

    def __init__(self, data, ld):
        S, rows, cols = data.shape
        self.whole = torch.full((S, rows, ld), SENT, dtype=torch.int32, device="cuda")
        self.whole[:, :, :cols] = torch.from_numpy(np.array(data, dtype=np.float32).view(np.int32)).cuda()

    def ptr(self):
        return self.whole.data_ptr()


class PlaneBuf:
    """Three bf16 planes [rows, cols] with leading dimension ldp inside sentinel rows and slack columns."""

    def __init__(self, rows, cols, ldp):
        self.rows, self.cols, self.ldp = rows, cols, ldp
        self.whole = torch.full((3, rows + 2 * PAD_ROWS, ldp), SENT16, dtype=torch.int16, device="cuda")
        self.stride = (rows + 2 * PAD_ROWS) * ldp

    def as_c(self, **over):
        from mmvae_amd import _lib

        return _lib.Planes(over.get("p", self.whole[0, PAD_ROWS].data_ptr()), over.get("ld", self.ldp),
                           over.get("plane_stride", self.stride))

    def planes(self):
        return self.whole[:, PAD_ROWS:PAD_ROWS + self.rows, :self.cols].cpu().numpy().view(np.uint16)

    def slack_untouched(self):
        w = self.whole
        return bool((w[:, :PAD_ROWS] == SENT16).all() and (w[:, PAD_ROWS + self.rows:] == SENT16).all()
                    and (w[:, :, self.cols:] == SENT16).all())

    def untouched(self):
        return bool((self.whole == SENT16).all())


def dev_u8(a):
    return None if a is None else _Raw(torch.from_numpy(np.array(a)).cuda())


class _Raw:
    def __init__(self, t):
        self.t = t

    def ptr(self):
        return self.t.data_ptr()


def workspace(B, N):
    from mmvae_amd import _lib

    nbytes = _lib.load().mmvae_fc_workspace_bytes(B, N)
    assert nbytes == 3 * R.n_chunks(B) * N * 4
    return Vec(nbytes // 4, pad=8 * N + 8), nbytes


def deviation(kind, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    if kind == "abs":
        return float(np.abs(got - want).max())
    norm = float(np.linalg.norm(want))
    return float(np.linalg.norm(got - want)) / (norm if norm > 0 else 1.0)


def held(family, name, kind, got, want, in_fp32, positive_delta=False):
    """dev <= 4 delta + floor; prints and records both figures.  Returns the bound."""
    dev, delta = deviation(kind, got, want), deviation(kind, in_fp32, want)
    bound = 4 * delta + (FLOOR_ABS if kind == "abs" else FLOOR_REL)
    print(f"  {family} {name}: device {dev:.3e}, the restatement in fp32 {delta:.3e} ({kind}), bound {bound:.3e}")
    if dev >= MAXIMA[family, name][0]:
        MAXIMA[family, name] = (dev, delta)
    assert np.isfinite(dev), name
    if positive_delta:
        assert delta > 0, name
    assert dev <= bound, (name, dev, delta)
    return bound


def slope_is_legitimate(slope, y64, bound_y):
    differ = slope != (y64 > 0)
    share = float(differ.mean())
    print(f"  slope: {int(differ.sum())} of {differ.size} differ from 1[y > 0] of the fp64 restatement")
    assert share <= 0.005, share
    assert not differ.any() or float(np.abs(y64[differ]).max()) <= bound_y, float(np.abs(y64[differ]).max())


@pytest.fixture(scope="module", autouse=True)
def summary():
    MAXIMA.clear()
    yield
    print("\nlargest deviation from the fp64 restatement per family and output (with that case's delta):")
    for (family, name), (dev, delta) in sorted(MAXIMA.items()):
        print(f"fc-tails-summary {family:24s} {name:14s} device {dev:.3e}  fp32 restatement {delta:.3e}")


# ------------------------------------------------------------------------------------------------------- column tail
def opt(flag, value):
    return value if flag else None


class ColumnRun:
    """Device buffers of one column case and the calls over them."""

    def __init__(self, case, data=None, inp=None, ld_in=None, ld_out=None):
        from mmvae_amd import _lib

        self.case, self.inp = case, FC.column_inputs(case, data) if inp is None else inp
        B, N, inp = case.B, case.N, self.inp
        self.ld_in, self.ld_out = ld_in or N + 3, ld_out or N + 5
        self.slabs, self.din = Slabs(inp["slabs"], self.ld_in), Slabs(inp["din"], self.ld_in)
        self.bias = opt(case.bias, Vec(N, inp["bias"]))
        self.gamma, self.beta = opt(case.bn and case.affine, Vec(N, inp["gamma"])), opt(case.bn and case.affine, Vec(N, inp["beta"]))
        self.rm, self.rv = opt(case.bn and case.running, Vec(N, inp["running_mean"])), opt(case.bn and case.running, Vec(N, inp["running_var"]))
        self.nbt = torch.tensor([-7, 41, -7], dtype=torch.int64, device="cuda") if case.bn and case.nbt else None
        p = lambda v: None if v is None else v.ptr()  # noqa: E731
        self.bn = None
        if case.bn:
            self.bn = _lib.BnParams(p(self.gamma), p(self.beta), p(self.rm), p(self.rv),
                                    None if self.nbt is None else self.nbt[1:].data_ptr(), FC.MOMENTUM, FC.BN_EPS)
        self.mask_np = opt(case.p > 0, inp["mask"])
        self.mask = dev_u8(self.mask_np)
        self.z, self.a, self.d = (Mat(B, N, self.ld_out) for _ in range(3))
        self.mean, self.invstd = Vec(N), Vec(N)
        self.ws, self.ws_bytes = workspace(B, N)
        self.addend = opt(case.addend, Mat(B, N, self.ld_out, inp["addend"]))
        self.addend_a = opt(case.addend_a, Mat(B, N, self.ld_out, inp["addend_a"]))
        self.row_scale = opt(case.row_scale, Vec(B, inp["row_scale"]))
        self.dz = Mat(B, N, self.ld_out)
        self.dbias, self.dgamma, self.dbeta = Vec(N), Vec(N), Vec(N)

    def buffers(self):
        return [v for v in vars(self).values() if isinstance(v, (Mat, PlaneBuf))]

    def fwd(self, training=True, mask=True, **over):
        c = self.case
        kw = dict(B=c.B, N=c.N, inp=self.slabs, ld_in=self.ld_in, n_slabs=c.S_fwd, bias=self.bias, bn=self.bn,
                  training=int(training), relu=int(c.relu), keep_mask=self.mask if mask else None,
                  dropout_p=c.p if mask else 0.0, z_out=self.z, a_out=self.a, d_out=self.d, ld_out=self.ld_out,
                  save_mean=opt(c.bn and training, self.mean), save_invstd=opt(c.bn and training, self.invstd),
                  workspace=self.ws, workspace_bytes=self.ws_bytes)
        kw.update(over)
        return call("mmvae_fc_epilogue_fwd", **kw)

    def bwd(self, **over):
        c = self.case
        kw = dict(B=c.B, N=c.N, din=self.din, ld_in=self.ld_in, n_slabs=c.S_bwd, addend=self.addend, addend_a=self.addend_a,
                  row_scale=self.row_scale, keep_mask=self.mask, dropout_p=c.p, relu=int(c.relu), a=opt(c.relu, self.a),
                  z=opt(c.bn, self.z), gamma=self.gamma, save_mean=opt(c.bn, self.mean), save_invstd=opt(c.bn, self.invstd),
                  has_bn=int(c.bn), dz_out=self.dz, ld_out=self.ld_out, dbias=self.dbias, dgamma=opt(c.bn, self.dgamma),
                  dbeta=opt(c.bn, self.dbeta), workspace=self.ws, workspace_bytes=self.ws_bytes)
        kw.update(over)
        return call("mmvae_fc_epilogue_bwd", **kw)

    def restate_fwd(self, dtype, training=True, mask=True):
        c, inp = self.case, self.inp
        return R.column_fwd(inp["slabs"], opt(c.bias, inp["bias"]), FC.column_bn(c, inp), training, c.relu,
                            self.mask_np if mask else None, c.p if mask else 0.0, dtype)

    def restate_bwd(self, dtype, fwd, slope):
        c, inp = self.case, self.inp
        return R.column_bwd(inp["din"], opt(c.bn, fwd), opt(c.bn and c.affine, inp["gamma"]), opt(c.addend, inp["addend"]),
                            opt(c.addend_a, inp["addend_a"]), opt(c.row_scale, inp["row_scale"]), self.mask_np, c.p, slope,
                            dtype)


def column_id(c):
    return f"{c.B}x{c.N}-s{c.S_fwd}-{c.S_bwd}-{'bn' if c.bn else 'plain'}"


@pytest.mark.parametrize("data", FC.DATA)
@pytest.mark.parametrize("case", FC.COLUMN_CASES, ids=column_id)
def test_column_tail_training_forward_and_backward(case, data):
    print(f"\n{case} {data}")
    run = ColumnRun(case, data)
    B, N = case.B, case.N
    family = f"column {'bn' if case.bn else 'plain'} {data}"
    positive = data == "offset" and B > 1
    f64, f32 = run.restate_fwd(np.float64), run.restate_fwd(np.float32)
    assert run.fwd() == 0
    # z: plain additions, bias first, then the slabs in order
    assert np.array_equal(run.z.bits(), f32["z"].view(np.uint32))
    a, d = run.a.get(), run.d.get()
    bound_y = held(family, "a", "abs", a, f64["a"], f32["a"], positive)
    held(family, "d", "abs", d, f64["d"], f32["d"], positive)
    if case.p > 0:
        assert not d[run.mask_np == 0].any()
    if case.relu:
        assert not a[f64["y"] < -bound_y].any() and not d[f64["y"] < -bound_y].any() and a.min() >= 0
    if case.bn:
        held(family, "save_mean", "abs", run.mean.get(), f64["mean"], f32["mean"], positive)
        held(family, "save_invstd", "abs", run.invstd.get(), f64["invstd"], f32["invstd"], positive)
        if case.running:
            held(family, "running_mean", "abs", run.rm.get(), f64["running_mean"], f32["running_mean"], positive)
            held(family, "running_var", "abs", run.rv.get(), f64["running_var"], f32["running_var"], positive)
        if case.nbt:
            assert run.nbt.tolist() == [-7, 42, -7]
    else:
        assert run.mean.untouched() and run.invstd.untouched() and run.ws.untouched()
    # backward, at the slope the device's forward pass left in a
    slope = (a > 0) if case.relu else None
    if case.relu:
        slope_is_legitimate(slope, f64["y"], bound_y)
    b64, b32 = run.restate_bwd(np.float64, f64, slope), run.restate_bwd(np.float32, f32, slope)
    assert run.bwd() == 0
    held(family, "dz", "rel", run.dz.get(), b64["dz"], b32["dz"], positive)
    if case.bn:
        held(family, "dgamma", "rel", run.dgamma.get(), b64["dgamma"], b32["dgamma"], positive)
        held(family, "dbeta", "rel", run.dbeta.get(), b64["dbeta"], b32["dbeta"], positive)
        dbias, rule = float(np.abs(run.dbias.get()).max()), 1e-3 * float(np.abs(b64["dy"]).max()) * B
        print(f"  {family} dbias ahead of the BatchNorm: largest {dbias:.3e} (the restatement in fp32 "
              f"{float(np.abs(b32['dbias']).max()):.3e}), bound {rule:.3e}")
        if dbias >= MAXIMA[family, "dbias / bound"][0]:
            MAXIMA[family, "dbias / bound"] = (dbias, rule)
        assert dbias <= rule
    else:
        held(family, "dbias", "rel", run.dbias.get(), b64["dbias"], b32["dbias"], positive)
        assert run.dgamma.untouched() and run.dbeta.untouched()
    assert all(buf.slack_untouched() for buf in run.buffers())


@pytest.mark.parametrize("data", FC.DATA)
@pytest.mark.parametrize("with_mask", [False, True], ids=["no mask", "mask"])
@pytest.mark.parametrize("case", FC.EVAL_CASES, ids=column_id)
def test_column_tail_eval_mode(case, with_mask, data):
    """Running statistics, with and without a keep mask; nothing but z, a and d is written."""
    print(f"\n{case} {data}")
    run = ColumnRun(case._replace(p=0.25), inp=FC.column_inputs(case, data))
    case = run.case
    f64, f32 = (run.restate_fwd(dt, training=False, mask=with_mask) for dt in (np.float64, np.float32))
    before = [v.whole.clone() for v in (run.rm, run.rv)]
    assert run.fwd(training=False, mask=with_mask) == 0
    family = f"column eval {data}"
    assert np.array_equal(run.z.bits(), f32["z"].view(np.uint32))
    positive = data == "offset" and case.B > 1  # (one element under a ReLU may be an exact zero)
    held(family, "a", "abs", run.a.get(), f64["a"], f32["a"], positive)
    held(family, "d", "abs", run.d.get(), f64["d"], f32["d"], positive)
    if with_mask:
        assert not run.d.get()[run.mask_np == 0].any()
    else:
        assert np.array_equal(run.d.bits(), run.a.bits())
    assert torch.equal(run.rm.whole, before[0]) and torch.equal(run.rv.whole, before[1])
    assert run.nbt is None or run.nbt.tolist() == [-7, 41, -7]
    assert run.mean.untouched() and run.invstd.untouched() and run.ws.untouched()
    assert all(buf.slack_untouched() for buf in run.buffers())
    # z_out and a_out are optional here: d alone gives the same bits
    d_alone = Mat(case.B, case.N, run.ld_out)
    assert run.fwd(training=False, mask=with_mask, z_out=None, a_out=None, d_out=d_alone) == 0
    assert np.array_equal(d_alone.bits(), run.d.bits()) and d_alone.slack_untouched()


@pytest.mark.parametrize("data", FC.DATA)
@pytest.mark.parametrize("S,bias,relu", [(1, False, True), (5, True, False)])
def test_one_row_under_training_batchnorm(S, bias, relu, data):
    """torch refuses a batch of one row under training BatchNorm; the C entry accepts it (include/mmvae_hip.h):
    save_mean = z, save_invstd = 1 / sqrt(eps), y = beta, running_var moves towards 0, and the backward pass gives dz = 0."""
    case = FC.ColumnCase(B=1, N=130, S_fwd=S, S_bwd=S, bn=True, bias=bias, affine=True, running=True, nbt=True, relu=relu,
                         p=0.0, addend=True, addend_a=False, row_scale=False)
    rng = np.random.default_rng([S, FC.DATA.index(data)])
    mu, sd = FC.column_means_and_stds(130) if data == "offset" else (np.zeros(130), np.ones(130))
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)  # noqa: E731
    inp = dict(slabs=f32(mu / S + sd * rng.standard_normal((S, 1, 130))), bias=f32(rng.standard_normal(130)),
               gamma=f32(1 + 0.1 * rng.standard_normal(130)), beta=f32(rng.standard_normal(130)),
               running_mean=f32(mu), running_var=f32(sd * sd), mask=np.ones((1, 130), np.uint8),
               din=f32(rng.standard_normal((S, 1, 130))), addend=f32(rng.standard_normal((1, 130))),
               addend_a=f32(np.zeros((1, 130))), row_scale=f32(np.ones(1)))
    one = np.float32(1)
    z = R.slab_sum(inp["slabs"], inp["bias"] if bias else None, np.float32)
    run = ColumnRun(case, inp=inp)
    assert run.fwd() == 0
    assert np.array_equal(run.z.bits(), z.view(np.uint32))
    assert np.array_equal(run.mean.bits()[0], z.view(np.uint32)[0])
    assert np.all(run.invstd.get() == one / np.sqrt(np.float32(FC.BN_EPS)))
    want_a = np.maximum(inp["beta"], 0) if relu else inp["beta"]
    assert np.array_equal(run.a.get()[0], want_a) and np.array_equal(run.d.get()[0], want_a)
    assert np.array_equal(run.rv.get(), (one - np.float32(FC.MOMENTUM)) * inp["running_var"])
    assert np.all(run.rv.get() < inp["running_var"])
    want_rm = (1 - FC.MOMENTUM) * inp["running_mean"].astype(np.float64) + FC.MOMENTUM * z[0].astype(np.float64)
    assert np.abs(run.rm.get() - want_rm).max() <= FLOOR_ABS + 2.0 ** -23 * np.abs(want_rm).max()
    assert run.nbt.tolist() == [-7, 42, -7]
    assert run.bwd() == 0
    assert not run.dz.get().any() and not run.dgamma.get().any()
    slope = (run.a.get() > 0) if relu else None
    dy = R.column_dy(inp["din"], inp["addend"], slope=slope, dtype=np.float32)
    assert np.array_equal(run.dbeta.get(), dy[0])
    assert all(buf.slack_untouched() for buf in run.buffers())


@pytest.mark.parametrize("B,N,bn", [(33, 65, False), (300, 130, False), (33, 65, True), (300, 130, True)])
def test_dz_out_may_alias_din_with_one_slab(B, N, bn):
    case = next(c for c in FC.COLUMN_CASES if c.bn == bn)._replace(B=B, N=N, S_fwd=1, S_bwd=1, relu=True, p=0.25,
                                                                     addend=True, addend_a=True, row_scale=True, affine=True)
    rng = np.random.default_rng([B, N, int(bn)])
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)  # noqa: E731
    inp = dict(slabs=f32(rng.standard_normal((1, B, N))), bias=f32(rng.standard_normal(N)),
               gamma=f32(1 + 0.1 * rng.standard_normal(N)), beta=f32(0.1 * rng.standard_normal(N)),
               running_mean=f32(np.zeros(N)), running_var=f32(np.ones(N)), mask=(rng.random((B, N)) >= 0.25).astype(np.uint8),
               din=f32(rng.standard_normal((1, B, N))), addend=f32(rng.standard_normal((B, N))),
               addend_a=f32(rng.standard_normal((B, N))), row_scale=f32(rng.random(B) + 0.5))
    ld = N + 5
    run = ColumnRun(case, inp=inp, ld_in=ld, ld_out=ld)
    assert run.fwd() == 0 and run.bwd() == 0
    separate = [buf.bits().copy() for buf in (run.dz, run.dbias, run.dgamma, run.dbeta)]
    assert np.isfinite(run.dz.get()).all()
    both = Mat(B, N, ld, inp["din"][0])  # din and dz_out in one buffer
    run.dbias, run.dgamma, run.dbeta = Vec(N), Vec(N), Vec(N)
    assert run.bwd(din=both, dz_out=both) == 0
    aliased = [buf.bits() for buf in (both, run.dbias, run.dgamma, run.dbeta)]
    for got, want in zip(aliased if bn else aliased[:2], separate):
        assert np.array_equal(got, want)
    assert both.slack_untouched()


@pytest.mark.parametrize("B,N,S", [(1, 1, 1), (33, 65, 5), (300, 130, 4), (513, 200, 7)])
def test_workspace_only_column_sum(B, N, S):
    """dz_out = dbias = NULL: the workspace receives the [ceil(B / 32)][N] column sums of each chunk and nothing else;
    a call with dbias adds them in chunk order; two runs give the same bits."""
    rng = np.random.default_rng([B, N, S])
    din = np.float32(rng.standard_normal((S, B, N)) + 0.25)
    row_scale = np.float32(rng.random(B) + 0.5)
    b64, b32 = (R.column_bwd(din, row_scale=row_scale, dtype=dt) for dt in (np.float64, np.float32))
    RC = R.n_chunks(B)
    slabs, rs = Slabs(din, N + 3), Vec(B, row_scale)
    runs = []
    for dbias in (None, Vec(N), Vec(N)):
        ws, nbytes = workspace(B, N)
        assert call("mmvae_fc_epilogue_bwd", B=B, N=N, din=slabs, ld_in=N + 3, n_slabs=S, row_scale=rs, ld_out=N + 5,
                    dbias=dbias, workspace=ws, workspace_bytes=nbytes) == 0
        parts = ws.bits()[0, :RC * N].reshape(RC, N)
        assert (ws.body[0, RC * N:] == SENT).all() and ws.slack_untouched()
        runs.append((parts, None if dbias is None else dbias.bits()))
        assert dbias is None or dbias.slack_untouched()
    parts = runs[0][0].view(np.float32)
    held("column plain centred", "chunk partials", "rel", parts, b64["partials"], b32["partials"])
    assert all(np.array_equal(runs[0][0], r[0]) for r in runs[1:])
    assert np.array_equal(runs[1][1], runs[2][1])
    assert np.array_equal(runs[1][1][0], R.in_chunk_order(parts).view(np.uint32))


@pytest.mark.parametrize("B,N", FC.PLANE_SHAPES)
def test_planes_off_a_multiple_of_64_columns(B, N):
    """d_planes / dz_planes: the planes are the exact three-way split of the fp32 output, the columns up to ldp and the
    rows around them untouched.  Forward behind a BatchNorm with a mask; backward with BatchNorm (the final dz, second
    launch) and without (first launch)."""
    ldp = N + 6
    for bn in (True, False):
        case = next(c for c in FC.COLUMN_CASES if c.bn == bn)._replace(B=B, N=N, S_fwd=4, S_bwd=5, relu=True, p=0.25,
                                                                         addend=True, affine=True)
        rng = np.random.default_rng([B, N, int(bn), 9])
        f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)  # noqa: E731
        inp = dict(slabs=f32(rng.standard_normal((4, B, N))), bias=f32(rng.standard_normal(N)),
                   gamma=f32(1 + 0.1 * rng.standard_normal(N)), beta=f32(0.1 * rng.standard_normal(N)),
                   running_mean=f32(np.zeros(N)), running_var=f32(np.ones(N)),
                   mask=(rng.random((B, N)) >= 0.25).astype(np.uint8), din=f32(rng.standard_normal((5, B, N))),
                   addend=f32(rng.standard_normal((B, N))), addend_a=f32(rng.standard_normal((B, N))),
                   row_scale=f32(rng.random(B) + 0.5))
        run = ColumnRun(case, inp=inp)
        assert run.fwd() == 0 and run.bwd() == 0
        plain = run.d.bits().copy(), run.dz.bits().copy()
        run.d, run.dz = Mat(B, N, run.ld_out), Mat(B, N, run.ld_out)
        dp, dzp = PlaneBuf(B, N, ldp), PlaneBuf(B, N, ldp)
        if bn:  # (the running statistics moved once: the second forward pass must not be compared through them)
            run.rm.set(inp["running_mean"]), run.rv.set(inp["running_var"])
        assert run.fwd(d_planes=dp.as_c()) == 0 and run.bwd(dz_planes=dzp.as_c()) == 0
        assert np.array_equal(run.d.bits(), plain[0]) and np.array_equal(run.dz.bits(), plain[1])
        assert np.array_equal(dp.planes(), R.x3_split(run.d.get())) and dp.slack_untouched()
        assert np.array_equal(dzp.planes(), R.x3_split(run.dz.get())) and dzp.slack_untouched()
        assert run.d.get().any() and run.dz.get().any()


# ----------------------------------------------------------------------------------------------- LayerNorm, row tail
@pytest.mark.parametrize("B,N", FC.LN_CASES)
def test_layernorm_entries(B, N):
    inp = FC.ln_inputs(B, N)
    f64, f32 = R.layernorm_fwd(inp["x"], FC.LN_EPS), R.layernorm_fwd(inp["x"], FC.LN_EPS, np.float32)
    x, y, mean, invstd = Mat(B, N, N + 1, inp["x"]), Mat(B, N, N + 2), Vec(B), Vec(B)
    print(f"\nlayernorm {B}x{N}")
    assert call("mmvae_layernorm_fwd", B=B, N=N, x=x, ldx=N + 1, eps=FC.LN_EPS, y=y, ldy=N + 2, save_mean=mean,
                save_invstd=invstd) == 0
    held("layernorm", "y", "abs", y.get(), f64["y"], f32["y"])
    held("layernorm", "save_mean", "abs", mean.get(), f64["mean"], f32["mean"])
    held("layernorm", "save_invstd", "abs", invstd.get(), f64["invstd"], f32["invstd"])
    if N == 1:
        assert not y.get().any() and np.all(invstd.get() == np.float32(1) / np.sqrt(np.float32(FC.LN_EPS)))
    # the backward pass reads the device's own y and invstd; the restatements read theirs
    g, dx = Mat(B, N, N + 4, inp["g"]), Mat(B, N, N + 3)
    assert call("mmvae_layernorm_bwd", B=B, N=N, dy=g, lddy=N + 4, y=y, ldy=N + 2, save_invstd=invstd, dx=dx,
                lddx=N + 3) == 0
    want = R.layernorm_bwd(inp["g"].astype(np.float64), f64["y"], f64["invstd"])
    held("layernorm", "dx", "rel", dx.get(), want, R.layernorm_bwd(inp["g"], f32["y"], f32["invstd"]))
    assert all(b.slack_untouched() for b in (x, y, mean, invstd, g, dx))
    # both saved vectors are optional
    y2 = Mat(B, N, N + 2)
    assert call("mmvae_layernorm_fwd", B=B, N=N, x=x, ldx=N + 1, eps=FC.LN_EPS, y=y2, ldy=N + 2) == 0
    assert np.array_equal(y2.bits(), y.bits())


@pytest.mark.parametrize("case", FC.ROW_CASES, ids=lambda c: f"{c.rows}x{c.N}-s{c.S_fwd}-{c.S_bwd}")
def test_row_tail_forward_and_backward(case):
    print(f"\n{case}")
    rows, N, inp = case.rows, case.N, FC.row_inputs(case)
    ld_in, ld_out = N + 3, N + 5
    mask_np = opt(case.p > 0, inp["mask"])
    bias_np = opt(case.bias, inp["bias"])
    f64, f32 = (R.rowtail_fwd(inp["slabs"], bias_np, FC.LN_EPS, case.relu, mask_np, case.p, dt) for dt in (np.float64, np.float32))
    slabs, bias, mask = Slabs(inp["slabs"], ld_in), opt(case.bias, Vec(N, inp["bias"])), dev_u8(mask_np)
    y, a, d, invstd = Mat(rows, N, ld_out), Mat(rows, N, ld_out), Mat(rows, N, ld_out), Vec(rows)
    fwd = dict(B=rows, N=N, inp=slabs, ld_in=ld_in, n_slabs=case.S_fwd, bias=bias, eps=FC.LN_EPS, relu=int(case.relu),
               ld_out=ld_out)
    assert call("mmvae_fc_rowtail_fwd", training=1, keep_mask=mask, dropout_p=case.p, y_out=y, a_out=a, d_out=d,
                save_invstd=invstd, **fwd) == 0
    bound_y = held("row tail", "y", "abs", y.get(), f64["y"], f32["y"])
    held("row tail", "a", "abs", a.get(), f64["a"], f32["a"])
    held("row tail", "d", "abs", d.get(), f64["d"], f32["d"])
    held("row tail", "save_invstd", "abs", invstd.get(), f64["invstd"], f32["invstd"])
    if mask_np is not None:
        assert not d.get()[mask_np == 0].any()
    if N == 1:
        assert not y.get().any() and np.all(invstd.get() == np.float32(1) / np.sqrt(np.float32(FC.LN_EPS)))
    # eval mode: no mask, nothing but d_out is written
    y_e, a_e, d_e, invstd_e = Mat(rows, N, ld_out), Mat(rows, N, ld_out), Mat(rows, N, ld_out), Vec(rows)
    assert call("mmvae_fc_rowtail_fwd", training=0, y_out=y_e, a_out=a_e, d_out=d_e, save_invstd=invstd_e, **fwd) == 0
    assert np.array_equal(d_e.bits(), a.bits()) and y_e.untouched() and a_e.untouched() and invstd_e.untouched()
    # backward at the device's slope
    slope = (a.get() > 0) if case.relu else None
    if case.relu:
        slope_is_legitimate(slope, f64["y"], bound_y)
    args = (opt(case.addend, inp["addend"]), opt(case.row_scale, inp["row_scale"]), mask_np, case.p, slope)
    b64, b32 = R.rowtail_bwd(inp["din"], f64, *args), R.rowtail_bwd(inp["din"], f32, *args, dtype=np.float32)
    din, addend = Slabs(inp["din"], ld_in), opt(case.addend, Mat(rows, N, ld_out, inp["addend"]))
    row_scale = opt(case.row_scale, Vec(rows, inp["row_scale"]))
    RC = R.n_chunks(rows)
    runs = []
    for _ in range(2):
        dz, dbias, ws = Mat(rows, N, ld_out), opt(not case.deferred, Vec(N)), Vec(RC * N, pad=8 * N + 8)
        assert call("mmvae_fc_rowtail_bwd", B=rows, N=N, din=din, ld_in=ld_in, n_slabs=case.S_bwd, addend=addend,
                    row_scale=row_scale, keep_mask=mask, dropout_p=case.p, relu=int(case.relu), act=opt(case.relu, a), y=y,
                    save_invstd=invstd, dz_out=dz, ld_out=ld_out, dbias=dbias, workspace=ws, workspace_bytes=RC * N * 4) == 0
        assert dz.slack_untouched() and ws.slack_untouched() and (dbias is None or dbias.slack_untouched())
        runs.append((dz.bits(), ws.bits()[0].reshape(RC, N), None if dbias is None else dbias.bits()[0]))
    dz, parts, dbias = runs[0]
    held("row tail", "dz", "rel", dz.view(np.float32), b64["dz"], b32["dz"])
    held("row tail", "chunk partials", "rel", parts.view(np.float32), b64["partials"], b32["partials"])
    if dbias is not None:
        assert np.array_equal(dbias, R.in_chunk_order(parts.view(np.float32)).view(np.uint32))
        assert np.array_equal(dbias, runs[1][2])
    assert np.array_equal(dz, runs[1][0]) and np.array_equal(parts, runs[1][1])
    assert all(b.slack_untouched() for b in (y, a, d, invstd, d_e))
    # without a workspace: the same dz, no bias gradient
    dz_only = Mat(rows, N, ld_out)
    assert call("mmvae_fc_rowtail_bwd", B=rows, N=N, din=din, ld_in=ld_in, n_slabs=case.S_bwd, addend=addend,
                row_scale=row_scale, keep_mask=mask, dropout_p=case.p, relu=int(case.relu), act=opt(case.relu, a), y=y,
                save_invstd=invstd, dz_out=dz_only, ld_out=ld_out) == 0
    assert np.array_equal(dz_only.bits(), dz) and dz_only.slack_untouched()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_six_entries_leaves_the_outputs_alone():
    """Each MMVAE_ERR_ARG / MMVAE_ERR_WORKSPACE condition written in the six entries, one call each, over outputs that
    hold sentinels before and after.  The unbroken argument lists are accepted (on other outputs) first."""
    from mmvae_amd import _lib

    ARG, WS = _lib.ERR_ARG, _lib.ERR_WORKSPACE
    B, N = 8, 16
    rng = np.random.default_rng(1)
    x = Mat(B, N, N, rng.standard_normal((B, N)))
    v = Vec(N, 1 + rng.random(N))
    vb = Vec(B, 1 + rng.random(B))
    m = dev_u8(np.ones((B, N), np.uint8))
    nbytes = _lib.load().mmvae_fc_workspace_bytes(B, N)

    def outputs():
        o = dict(z=Mat(B, N, N), a=Mat(B, N, N), d=Mat(B, N, N), mean=Vec(N), invstd=Vec(N), ws=workspace(B, N)[0],
                 rm=Vec(N), rv=Vec(N), dz=Mat(B, N, N), dbias=Vec(N), dgamma=Vec(N), dbeta=Vec(N), rows=Vec(B), rows2=Vec(B),
                 planes=PlaneBuf(B, N, N), sp=PlaneBuf(B, N, N))
        return o

    def lists(o):
        """the accepted argument lists over the outputs `o`"""
        bn = _lib.BnParams(v.ptr(), v.ptr(), o["rm"].ptr(), o["rv"].ptr(), None, 0.01, 1e-3)
        return bn, {
            "mmvae_fc_epilogue_fwd": dict(B=B, N=N, inp=x, ld_in=N, n_slabs=1, bias=v, bn=bn, training=1, relu=1, keep_mask=m,
                                          dropout_p=0.25, z_out=o["z"], a_out=o["a"], d_out=o["d"], ld_out=N,
                                          save_mean=o["mean"], save_invstd=o["invstd"], workspace=o["ws"],
                                          workspace_bytes=nbytes),
            "mmvae_fc_epilogue_bwd": dict(B=B, N=N, din=x, ld_in=N, n_slabs=1, keep_mask=m, dropout_p=0.25, relu=1, a=x, z=x,
                                          gamma=v, save_mean=v, save_invstd=v, has_bn=1, dz_out=o["dz"], ld_out=N,
                                          dbias=o["dbias"], dgamma=o["dgamma"], dbeta=o["dbeta"], workspace=o["ws"],
                                          workspace_bytes=nbytes),
            "mmvae_layernorm_fwd": dict(B=B, N=N, x=x, ldx=N, eps=1e-5, y=o["d"], ldy=N, save_mean=o["rows"],
                                        save_invstd=o["rows2"]),
            "mmvae_layernorm_bwd": dict(B=B, N=N, dy=x, lddy=N, y=x, ldy=N, save_invstd=vb, dx=o["dz"], lddx=N),
            "mmvae_fc_rowtail_fwd": dict(B=B, N=N, inp=x, ld_in=N, n_slabs=1, bias=v, eps=1e-5, training=1, relu=1,
                                         keep_mask=m, dropout_p=0.25, y_out=o["z"], a_out=o["a"], d_out=o["d"], ld_out=N,
                                         save_invstd=o["rows"]),
            "mmvae_fc_rowtail_bwd": dict(B=B, N=N, din=x, ld_in=N, n_slabs=1, keep_mask=m, dropout_p=0.25, relu=1, act=x, y=x,
                                         save_invstd=vb, dz_out=o["dz"], ld_out=N, dbias=o["dbias"], workspace=o["ws"],
                                         workspace_bytes=N * 4),
        }

    scratch = outputs()
    scratch["rm"].set(np.zeros(N)), scratch["rv"].set(np.ones(N))
    _, good = lists(scratch)
    for name, kw in good.items():
        assert call(name, **kw) == 0, name
    assert call("mmvae_fc_epilogue_fwd", **dict(good["mmvae_fc_epilogue_fwd"], d_planes=scratch["planes"].as_c())) == 0
    assert call("mmvae_fc_epilogue_bwd", **dict(good["mmvae_fc_epilogue_bwd"], dz_planes=scratch["planes"].as_c())) == 0
    split = _lib.SplitJob(B, N, x.ptr(), N, scratch["sp"].as_c())
    assert call("mmvae_fc_epilogue_fwd", **dict(good["mmvae_fc_epilogue_fwd"], split=split)) == 0

    o = outputs()
    bn, base = lists(o)
    pl, sp = o["planes"], o["sp"]
    no_rm = _lib.BnParams(v.ptr(), v.ptr(), None, o["rv"].ptr(), None, 0.01, 1e-3)
    no_rv = _lib.BnParams(v.ptr(), v.ptr(), o["rm"].ptr(), None, None, 0.01, 1e-3)
    job = lambda **k: _lib.SplitJob(k.pop("rows", B), k.pop("cols", N), k.pop("src", x.ptr()), k.pop("ld_src", N),  # noqa: E731
                                    sp.as_c(**k))
    common = [(dict(B=0), ARG), (dict(N=0), ARG), (dict(n_slabs=0), ARG), (dict(ld_in=N - 1), ARG), (dict(ld_out=N - 1), ARG)]
    p_range = [(dict(dropout_p=1.0), ARG), (dict(dropout_p=-0.125), ARG)]
    planes_fwd = [(dict(d_planes=pl.as_c(), d_out=None, keep_mask=None), ARG), (dict(d_planes=pl.as_c(), N=N - 1), ARG),
                  (dict(d_planes=pl.as_c(ld=N - 2)), ARG), (dict(d_planes=pl.as_c(ld=N + 1)), ARG),
                  (dict(d_planes=pl.as_c(plane_stride=B * N - 2)), ARG)]
    planes_bwd = [(dict(dz_planes=pl.as_c(), dz_out=None, has_bn=0), ARG), (dict(dz_planes=pl.as_c(), N=N - 1), ARG),
                  (dict(dz_planes=pl.as_c(ld=N - 2)), ARG), (dict(dz_planes=pl.as_c(ld=N + 1)), ARG),
                  (dict(dz_planes=pl.as_c(plane_stride=B * N - 2)), ARG)]
    split_jobs = [(dict(split=job(), d_planes=pl.as_c()), ARG), (dict(split=job(p=None)), ARG), (dict(split=job(rows=0)), ARG),
                  (dict(split=job(cols=0)), ARG), (dict(split=job(src=None)), ARG), (dict(split=job(ld_src=N - 1)), ARG),
                  (dict(split=job(ld=N - 8)), ARG), (dict(split=job(ld=N + 4)), ARG),
                  (dict(split=job(plane_stride=sp.stride + 4)), ARG), (dict(split=job(plane_stride=B * N - 8)), ARG),
                  (dict(split=job(p=sp.as_c().p + 2)), ARG)]
    refusals = {
        "mmvae_fc_epilogue_fwd": common + p_range + planes_fwd + split_jobs + [
            (dict(inp=None), ARG), (dict(a_out=None, d_out=None, keep_mask=None), ARG), (dict(d_out=None), ARG),
            (dict(z_out=None), ARG), (dict(save_mean=None), ARG), (dict(save_invstd=None), ARG),
            (dict(training=0, bn=no_rm), ARG), (dict(training=0, bn=no_rv), ARG),
            (dict(workspace=None), WS), (dict(workspace_bytes=nbytes - 1), WS)],
        "mmvae_fc_epilogue_bwd": common + p_range + planes_bwd + [
            (dict(din=None), ARG), (dict(a=None), ARG), (dict(z=None), ARG), (dict(save_mean=None), ARG),
            (dict(save_invstd=None), ARG), (dict(dz_out=None), ARG),
            (dict(has_bn=0, dz_out=None, dbias=None, workspace=None), ARG),
            (dict(workspace=None), WS), (dict(workspace_bytes=nbytes - 1), WS), (dict(has_bn=0, workspace=None), WS),
            (dict(has_bn=0, dbias=None, workspace_bytes=nbytes - 1), WS)],
        "mmvae_layernorm_fwd": [(dict(B=0), ARG), (dict(N=0), ARG), (dict(x=None), ARG), (dict(y=None), ARG),
                                (dict(ldx=N - 1), ARG), (dict(ldy=N - 1), ARG)],
        "mmvae_layernorm_bwd": [(dict(B=0), ARG), (dict(N=0), ARG), (dict(dy=None), ARG), (dict(y=None), ARG),
                                (dict(save_invstd=None), ARG), (dict(dx=None), ARG), (dict(lddy=N - 1), ARG),
                                (dict(ldy=N - 1), ARG), (dict(lddx=N - 1), ARG)],
        "mmvae_fc_rowtail_fwd": common + p_range + [
            (dict(inp=None), ARG), (dict(d_out=None), ARG), (dict(eps=-1.0), ARG), (dict(eps=float("nan")), ARG),
            (dict(training=0), ARG), (dict(save_invstd=None), ARG)],
        "mmvae_fc_rowtail_bwd": common + p_range + [
            (dict(din=None), ARG), (dict(y=None), ARG), (dict(save_invstd=None), ARG), (dict(dz_out=None), ARG),
            (dict(act=None), ARG), (dict(workspace=None), WS), (dict(workspace_bytes=N * 4 - 1), WS),
            (dict(dbias=None, workspace_bytes=0), WS)],
    }
    for name, cases in refusals.items():
        for over, code in cases:
            assert call(name, **dict(base[name], **over)) == code, (name, over)
    assert all(buf.untouched() for buf in o.values()), [k for k, buf in o.items() if not buf.untouched()]
