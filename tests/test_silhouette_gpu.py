"""GPU checks of libmmvae_sil.so (include/mmvae_sil.h) against the independent fp64 restatement
(tests/sil_restatement.py).  Both sides read the same fp32 rows, sorted into runs by the restatement's own helper
(`sorted_runs`), not by `mmvae_amd.silhouette.sort_runs`.

Shapes (N, D, classes, groups): (5, 3, 2, 1) N below the 64-row tile; (70, 8, 3, 1) just past one tile, several runs
inside one column tile; (400, 16, 2, 1) runs of about 200 rows that span several tiles; (300, 70, 5, 3) and
(1030, 130, 7, 4) D off 4 and off 64, two and three 64-column chunks, groups around a row tile; (200, 512, 4, 2) the largest
D.  Both metrics, and two kinds of data: Gaussian clusters, and the same with every cell of class 0 a copy of one row.
Every case also plants a class of a single cell (a = 0, s = 0), a group with a single class (b NaN, nearest -1, s NaN),
ldx = D + 5 with NaN in the pad columns, and PAD sentinel elements around every output.

Bounds on |a - a64| and |b - b64| (delta):

  cosine      (2 D + 136) 2^-24: the kNN header's pair bound (2 D + 8) 2^-24, 63 fp32 additions of a tile partial on
              means <= 2 (2 x 63 x 2^-24 rounded up to 128 x 2^-24 together with the fp32 store).
  Euclidean   EUCLID_REL x the case's largest mean distance.  The Gram form n_i + n_j - 2 g_ij has an error of its own,
              measured with `sil_restatement.gram_form_fp32` (the formula in fp32 numpy on the centred rows, bit-equal
              rows at distance 0, means in fp64) against the restatement, relative to the largest mean distance:

                  (N, D)          clusters    duplicates
                  (5, 3)          3.5e-08     3.2e-08
                  (70, 8)         2.1e-07     7.3e-08
                  (400, 16)       1.3e-07     4.4e-08
                  (300, 70)       3.1e-07     2.6e-07
                  (1030, 130)     6.9e-07     4.4e-07
                  (200, 512)      6.2e-07     1.14e-06

              (It grows with D as the fp32 chain's error does, times (n_i + n_j) / d^2 -- about 6 for two cells of one
              of these clusters.)  The kernel gets 8 x the largest of these for its other summation order:
              EUCLID_REL = 8 x 1.14e-06 = 9.1e-06.  On the MI355X the kernel's own error is 3e-8 .. 1.2e-6 of the
              scale at these shapes: the formula's, not more.  With the norms taken from a separate row pass instead of the Gram chain, a duplicated
              class shows up to 3.2e-4 here (the square root of a cancellation residue), which is why the header has the
              exact-zero rule; the test asks a == 0 exactly there.

s: where max(a64, b64) > 0, |s - s64| <= 2 (delta_a + delta_b) / max(a64, b64) + 2^-23; NaN exactly where the restatement
has it.  nearest: equal wherever the restatement's lead exceeds 4 delta_b; at most 1 % of the rows may be left out.
Cosine results are checked a second time against the identity sum_{j in c} d(i, j) = n_c - <u_i, sum_{j in c} u_j>.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from tests import sil_restatement as R

pytestmark = pytest.mark.gpu

PAD = 8  # sentinel elements in front of and behind every output
EUCLID_REL = 8 * 1.14e-6
SHAPES = [(5, 3, 2, 1), (70, 8, 3, 1), (400, 16, 2, 1), (300, 70, 5, 3), (1030, 130, 7, 4), (200, 512, 4, 2)]
METRICS = ["euclidean", "cosine"]
KINDS = ["clusters", "duplicates"]


def make_case(N, D, C, G, metric, kind):
    """(fp32 rows in run order, class, group of every row, run_ptr, run_group, run_class, index of the planted single
    cell, indices of the planted one-class group): what both sides read."""
    seed = 1000 * D + N
    X, cls = R.clusters(seed, N, D, C)
    rng = np.random.default_rng(seed + 1)
    group = rng.integers(0, G, N).astype(np.int32)
    cls[:5] = [0, 0, 0, 1, 0]                 # (N = 5: classes 0 and 1 both live beside the planted cells)
    cls[0], group[0] = C, group[2]            # a class of a single cell, in the group of cells 2 .. 4
    group[3:5] = group[2]
    lone = np.arange(1, 2 if N == 5 else 4)
    cls[lone], group[lone] = 0, G             # a group with a single class
    if kind == "duplicates":
        X = R.with_duplicates(X, cls, 0)
    if metric == "euclidean":
        X = X - X.mean(0, keepdims=True)      # the centring of silhouette_samples (bit-equal rows stay bit-equal)
    X32 = X.astype(np.float32)
    order, run_ptr, run_group, run_class = R.sorted_runs(cls, group)
    single = int(np.nonzero(order == 0)[0][0])
    alone = np.nonzero(np.isin(order, lone))[0]
    return X32[order], cls[order], group[order], run_ptr, run_group, run_class, single, alone


def bounds(D, metric, a64, b64):
    if metric == "cosine":
        return (2 * D + 136) * 2.0 ** -24
    return EUCLID_REL * max(np.nanmax(a64), np.nanmax(b64))


@functools.lru_cache(maxsize=None)
def reference(N, D, C, G, metric, kind):
    """Inputs and the restatement's results of one case; computed once and never written to."""
    X, cls, group, run_ptr, run_group, run_class, single, alone = make_case(N, D, C, G, metric, kind)
    a, b, s, nearest, lead = R.silhouette(X, cls, group, metric)
    out = dict(X=X, cls=cls, group=group, run_ptr=run_ptr, run_group=run_group, run_class=run_class, a=a, b=b, s=s,
               nearest=nearest, lead=lead, alone=alone)
    for v in out.values():
        v.setflags(write=False)
    out["single"] = single
    return out


def _lib():
    from mmvae_amd import _sil_lib

    return _sil_lib, _sil_lib.load_sil()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Padded:
    """An output buffer with PAD sentinel elements on both sides of its `n` elements."""

    def __init__(self, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.whole = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device="cuda")
        self.body = self.whole[PAD:PAD + n]

    def ptr(self):
        return self.body.data_ptr()

    def untouched_outside(self):
        return bool((self.whole[:PAD] == self.sentinel).all() and (self.whole[PAD + self.n:] == self.sentinel).all())

    def untouched(self):
        return bool((self.whole == self.sentinel).all())


def run_device(X, metric, run_ptr, run_group, extra_ld=5):
    """The C entry on rows with leading dimension D + extra_ld (NaN in the pad columns), into sentinel-padded outputs and
    a workspace of exactly the asked size followed by sentinel bytes.  Returns numpy results; checks the sentinels."""
    L, lib = _lib()
    N, D = X.shape
    wide = torch.full((N, D + extra_ld), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :D] = torch.from_numpy(np.array(X)).cuda()
    ptr_d, group_d = torch.from_numpy(np.array(run_ptr)).cuda(), torch.from_numpy(np.array(run_group)).cuda()
    a, b, s = (Padded(N, torch.float32, -5.0) for _ in range(3))
    nearest = Padded(N, torch.int32, -99)
    nbytes = lib.mmvae_sil_rows_workspace_bytes(N, D)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    L.check(lib.mmvae_sil_rows_f32(N, D, wide.data_ptr(), D + extra_ld, {"euclidean": 0, "cosine": 1}[metric],
                                   len(run_group), ptr_d.data_ptr(), group_d.data_ptr(), a.ptr(), b.ptr(), nearest.ptr(),
                                   s.ptr(), ws.data_ptr(), nbytes, _stream()), "mmvae_sil_rows_f32")
    torch.cuda.synchronize()
    for name, buf in (("a", a), ("b", b), ("s", s), ("nearest", nearest)):
        assert buf.untouched_outside(), f"{name}: written outside its rows"
    assert bool((ws[nbytes:] == 0xAB).all()), "written past the workspace"
    return dict(a=a.body.cpu().numpy(), b=b.body.cpu().numpy(), s=s.body.cpu().numpy(),
                nearest=nearest.body.cpu().numpy())


def check_against(got, ref, delta, what=""):
    """The module docstring's assertions on (a, b, s, nearest) against restatement values in the same row order."""
    a64, b64, s64 = ref["a"], ref["b"], ref["s"]
    err_a = np.abs(got["a"] - a64)
    err_b = np.abs(got["b"] - b64)
    top = np.fmax(a64, b64)
    tol_s = 2 * (2 * delta) / np.where(top > 0, top, 1.0) + 2.0 ** -23
    err_s = np.abs(got["s"] - s64)
    print(f"{what}: delta {delta:.3e}, |a - a64| max {np.nanmax(err_a):.3e}, |b - b64| max "
          f"{np.nanmax(err_b) if np.isfinite(b64).any() else 0.0:.3e}, |s - s64| max "
          f"{np.nanmax(err_s) if np.isfinite(s64).any() else 0.0:.3e} (smallest allowance {np.nanmin(tol_s):.3e}), "
          f"lead min {np.min(ref['lead']):.3e}")
    assert np.array_equal(np.isnan(got["a"]), np.isnan(a64)) and (err_a[~np.isnan(a64)] <= delta).all()
    assert np.array_equal(np.isnan(got["b"]), np.isnan(b64)) and (err_b[~np.isnan(b64)] <= delta).all()
    assert np.array_equal(np.isnan(got["s"]), np.isnan(s64))
    live = ~np.isnan(s64) & (top > 0)
    assert (err_s[live] <= tol_s[live]).all()
    assert (got["s"][~np.isnan(s64) & ~(top > 0)] == 0).all()
    sure = ref["lead"] > 4 * delta
    assert sure.mean() >= 0.99, f"{(~sure).sum()} rows are not sure of their nearest class"
    assert np.array_equal(got["nearest"][sure], ref["nearest"][sure])
    assert np.array_equal(got["nearest"] < 0, ref["nearest"] < 0)


def cosine_identity(X, run_ptr, run_group):
    """(a, b) fp64 of the cosine metric by sum_{j in c} d(i, j) = n_c - <u_i, sum_{j in c} u_j>: O(N D C), no pairs."""
    X = X.astype(np.float64)
    norm = np.sqrt((X * X).sum(1))
    U = X * np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 0.0)[:, None]
    R_ = len(run_group)
    counts = np.diff(run_ptr).astype(np.float64)
    S = np.stack([U[run_ptr[r]:run_ptr[r + 1]].sum(0) for r in range(R_)])
    run_of = np.repeat(np.arange(R_), np.diff(run_ptr))
    dots = U @ S.T
    N = len(X)
    a, b = np.zeros(N), np.full(N, np.nan)
    for i in range(N):
        r = run_of[i]
        if counts[r] > 1:
            a[i] = (counts[r] - 1 - (dots[i, r] - U[i] @ U[i])) / (counts[r] - 1)
        others = [(counts[q] - dots[i, q]) / counts[q] for q in range(R_) if q != r and run_group[q] == run_group[r]]
        if others:
            b[i] = min(others)
    return a, b


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N, D, C, G", SHAPES)
def test_entry_matches_the_restatement(N, D, C, G, metric, kind):
    ref = reference(N, D, C, G, metric, kind)
    got = run_device(ref["X"], metric, ref["run_ptr"], ref["run_group"])
    got["nearest"] = np.where(got["nearest"] >= 0, ref["run_class"][np.maximum(got["nearest"], 0)], -1)
    delta = bounds(D, metric, ref["a"], ref["b"])
    check_against(got, ref, delta, f"{kind} {metric} N={N} D={D}")
    # the planted cells
    i = ref["single"]
    assert got["a"][i] == 0 and got["s"][i] == 0 and got["b"][i] > 0 and got["nearest"][i] >= 0
    for j in ref["alone"]:
        assert np.isnan(got["b"][j]) and np.isnan(got["s"][j]) and got["nearest"][j] == -1 and got["a"][j] >= 0
    if kind == "duplicates":
        zero = ref["cls"] == 0
        assert zero.sum() > 1 or N == 5
        if metric == "euclidean":
            assert (got["a"][zero] == 0).all(), "bit-equal rows must be at distance exactly 0"
    if metric == "cosine":
        ia, ib = cosine_identity(ref["X"], ref["run_ptr"], ref["run_group"])
        assert (np.abs(got["a"] - ia) <= delta).all()
        assert (np.abs(got["b"] - ib)[~np.isnan(ib)] <= delta).all() and np.array_equal(np.isnan(ib), np.isnan(got["b"]))
    # a second call gives the same bits, with ldx = D as well
    again = run_device(ref["X"], metric, ref["run_ptr"], ref["run_group"], extra_ld=0)
    for name in ("a", "b", "s"):
        assert np.array_equal(again[name], got[name], equal_nan=True), name
    again["nearest"] = np.where(again["nearest"] >= 0, ref["run_class"][np.maximum(again["nearest"], 0)], -1)
    assert np.array_equal(again["nearest"], got["nearest"])


def test_refusals_leave_the_outputs_untouched():
    L, lib = _lib()
    N, D, R_ = 40, 6, 3
    x = torch.zeros((N, D), dtype=torch.float32, device="cuda")
    run_ptr = torch.tensor([0, 10, 25, 40], dtype=torch.int32, device="cuda")
    run_group = torch.zeros(3, dtype=torch.int32, device="cuda")
    a, b, s = (Padded(N, torch.float32, -5.0) for _ in range(3))
    nearest = Padded(N, torch.int32, -99)
    nbytes = lib.mmvae_sil_rows_workspace_bytes(N, D)
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    ok = [N, D, x.data_ptr(), D, 0, R_, run_ptr.data_ptr(), run_group.data_ptr(), a.ptr(), b.ptr(), nearest.ptr(), s.ptr(),
          ws.data_ptr(), nbytes, _stream()]
    bad = [{0: 0}, {1: 0}, {1: 513}, {3: D - 1}, {4: 2}, {4: -1}, {5: 0}, {5: N + 1}, {13: nbytes - 1},
           {12: ws.data_ptr() + 4}] + [{i: None} for i in (2, 6, 7, 8, 9, 10, 11, 12)]
    refused = [lib.mmvae_sil_rows_f32(*[change.get(i, v) for i, v in enumerate(ok)]) for change in bad]
    torch.cuda.synchronize()
    assert refused == [L.ERR_ARG] * len(bad), refused
    for name, buf in (("a", a), ("b", b), ("s", s), ("nearest", nearest)):
        assert buf.untouched(), name
    assert bool((ws == 0xAB).all())


@pytest.mark.parametrize("metric", METRICS)
def test_silhouette_samples_on_unsorted_rows_with_unlabelled_cells(metric):
    from mmvae_amd import silhouette

    N, D, C, G = 300, 70, 5, 3
    X, cls = R.clusters(77, N, D, C)
    rng = np.random.default_rng(78)
    group = rng.integers(0, G, N).astype(np.int32)
    cls[rng.random(N) < 0.1] = -1
    group[rng.random(N) < 0.05] = -1
    X32 = X.astype(np.float32)  # not centred: +3 in every coordinate
    a64, b64, s64, nearest64, lead = R.silhouette(X32, cls, group, metric)
    x = torch.from_numpy(X32).cuda()
    got = silhouette.silhouette_samples(x, torch.from_numpy(cls).cuda(), torch.from_numpy(group).cuda(), metric)
    assert all(t.is_cuda and t.shape == (N,) for t in got) and got.nearest.dtype == torch.int32
    delta = bounds(D, metric, a64, b64)
    if metric == "euclidean":
        # the rows the kernel reads are the fp64-centred rows rounded to fp32: every coordinate moves by at most
        # 2^-25 |x_c|, a row by sqrt(D) times that, a distance by two rows' worth
        kept = (cls >= 0) & (group >= 0)
        centred = X32[kept].astype(np.float64) - X32[kept].astype(np.float64).mean(0)
        delta += 2.0 ** -24 * np.sqrt(D) * np.abs(centred).max()
    dropped = (cls < 0) | (group < 0)
    assert dropped.sum() > 10 and np.isnan(a64[dropped]).all()
    check_against({k: getattr(got, k).cpu().numpy() for k in ("a", "b", "s", "nearest")},
                  dict(a=a64, b=b64, s=s64, nearest=nearest64, lead=lead), delta, f"silhouette_samples {metric}")
    assert (got.nearest.cpu().numpy()[dropped] == -1).all()
    one_group = silhouette.silhouette_samples(x, torch.from_numpy(cls).cuda(), None, metric)
    a1, b1, s1, n1, lead1 = R.silhouette(X32, cls, None, metric)
    check_against({k: getattr(one_group, k).cpu().numpy() for k in ("a", "b", "s", "nearest")},
                  dict(a=a1, b=b1, s=s1, nearest=n1, lead=lead1), delta, f"silhouette_samples {metric}, one group")
    with pytest.raises(ValueError, match="metric"):
        silhouette.silhouette_samples(x, torch.from_numpy(cls).cuda(), None, "manhattan")
    with pytest.raises(TypeError, match="float32"):
        silhouette.silhouette_samples(x.double(), torch.from_numpy(cls).cuda(), None, "cosine")


def _three_clusters():
    X, cluster = R.clusters(31, 240, 12, 3)
    meta = pd.DataFrame({"species": np.where(np.arange(240) % 2 == 0, "human", "mouse"),
                         "cell_type": np.array(["B", "NK", "T"], dtype=object)[cluster]})
    meta.loc[5, "cell_type"] = np.nan
    return X.astype(np.float32), meta


def test_silhouette_widths_tables_equal_the_restatement():
    from mmvae_amd import silhouette

    X32, meta = _three_clusters()
    out = silhouette.silhouette_widths(torch.from_numpy(X32).cuda(), meta)
    assert out.columns == ("species", "cell_type") and out.codes.shape == (2, 240) and out.metric == "euclidean"
    batch = pd.factorize(meta["species"], sort=True)[0].astype(np.int32)
    label = pd.factorize(meta["cell_type"], sort=True)[0].astype(np.int32)
    assert np.array_equal(out.codes.cpu().numpy(), np.stack([batch, label])) and label[5] == -1
    a_l, b_l, s_label, _, _ = R.silhouette(X32, label, None)
    a_b, b_b, s_batch, _, _ = R.silhouette(X32, batch, label)
    # every cell's s is within 2 (2 delta) / max(a, b) + 2^-23 (delta as in the test above, centring included); a mean of
    # such values, and of 1 - |s|, moves by no more than the largest allowance
    centred = X32.astype(np.float64) - X32.astype(np.float64).mean(0)
    tol = 0.0
    for a64, b64 in ((a_l, b_l), (a_b, b_b)):
        delta = bounds(12, "euclidean", a64, b64) + 2.0 ** -24 * np.sqrt(12) * np.abs(centred).max()
        top = np.fmax(a64, b64)
        tol = max(tol, float(np.nanmax(4 * delta / top[top > 0])) + 2.0 ** -23)
    assert tol < 1e-3
    assert tuple(out.summary.columns) == silhouette.SUMMARY_COLUMNS
    assert out.summary["column"].tolist() == ["cell_type"] * 2 and out.summary["role"].tolist() == ["label", "batch"]
    assert out.summary["n_classes"].tolist() == [3, 3] and out.summary["n_cells"].tolist() == [239, 239]
    want_label, want_batch = R.asw_label(s_label), R.asw_batch(s_batch, label, batch)
    assert abs(out.summary["asw"][0] - want_label) <= tol and abs(out.summary["asw"][1] - want_batch) <= tol
    assert abs(out.summary["scaled"][0] - (want_label + 1) / 2) <= tol and out.summary["scaled"][1] == out.summary["asw"][1]
    assert want_label > 0.3 and want_batch > 0.9  # three separate clusters, the species alternating inside them
    frame = pd.DataFrame({"label": label, "batch": batch, "s_label": s_label, "w": 1 - np.abs(s_batch)})[label >= 0]
    by = frame.groupby("label")
    table = out.per_label["cell_type"]
    assert tuple(table.columns) == silhouette.PER_LABEL_COLUMNS and table.index.tolist() == ["B", "NK", "T"]
    assert table["n_cells"].tolist() == by.size().tolist() and table["n_batches"].tolist() == by["batch"].nunique().tolist()
    assert np.abs(table["label_asw"].values - by["s_label"].mean().values).max() <= tol
    assert np.abs(table["batch_asw"].values - by["w"].mean().values).max() <= tol
    assert silhouette.asw_label(out.label_rows["cell_type"].s) == out.summary["asw"][0]
    assert silhouette.asw_batch(out.batch_rows["cell_type"].s, out.codes[1], out.codes[0]) == out.summary["asw"][1]


def test_trainer_silhouette_widths_on_the_smallest_golden_case(tmp_path, monkeypatch):
    from mmvae_amd import silhouette
    from mmvae_amd.constants import REGISTRY_KEYS as RK
    from mmvae_amd.trainer import Trainer
    from tests import helpers as H
    from tests import mirror_utils as MU

    case, z = H.load_case("two_mod_odd")
    model = MU.build_mirror(case, "cuda", str(tmp_path), use_engine=True)
    T = len(case["schedule"]) - 1
    MU.load_state(model, z, f"step{T}/sd/")
    x, _, _, _ = H.step_inputs(z, T)
    x = x.cuda()
    eid = str(z["eval/expert_id"])
    B = x.shape[0]
    frame = lambda g: pd.DataFrame({"group": [g] * B, "donor": [f"d{i % 2}" for i in range(B)]})  # noqa: E731
    batches = [(x, frame("a"), eid), (x.flip(0) * 0.5, frame("b"), eid)]
    trainer = Trainer()
    predictions = trainer.predict(model, batches)
    assert len(predictions) == 2 and predictions[0][RK.Z][0].shape[0] == B
    monkeypatch.setattr(trainer, "predict", lambda m, b: predictions)  # the same latent samples for both calls below
    out = trainer.silhouette_widths(model, batches, batch_key="donor", label_keys=("group",))
    assert isinstance(out, silhouette.SilhouetteWidths) and out.codes.shape == (2, 2 * B)
    rows = out.label_rows["group"]
    assert all(t.shape == (2 * B,) and t.is_cuda for t in rows) and bool(torch.isfinite(rows.s).all())
    assert bool(torch.isfinite(out.batch_rows["group"].s).all()) and bool(((rows.s >= -1) & (rows.s <= 1)).all())
    assert out.summary["role"].tolist() == ["label", "batch"] and np.isfinite(out.summary["asw"]).all()
    outs = [p[RK.Z] for p in predictions]
    direct = silhouette.silhouette_widths(torch.cat([o[0] for o in outs], 0),
                                          pd.concat([o[1] for o in outs], ignore_index=True), "donor", ("group",))
    assert direct.summary.equals(out.summary) and direct.per_label["group"].equals(out.per_label["group"])
