"""GPU checks of libmmvae_clust.so (include/mmvae_clust.h) and mmvae_amd.clustering against the independent fp64
restatement (tests/kmeans_restatement.py).  Both sides read the same fp32 rows and centroids.

Shapes (N, D, C): (5, 3, 2) below one row tile; (70, 8, 3) just past one; (300, 70, 5) D off 4, two column chunks;
(1030, 130, 7) D off 64, several slabs; (200, 512, 4) the largest D; (600, 16, 256) the largest C; (2100, 128, 37) the
production D with an odd C.  The rows are the Gaussian clusters of `sil_restatement.clusters` (min(C, 8) blobs), centred
and rounded to fp32; the centroids C distinct rows plus 0.3 N(0, 1) noise.  Every call has ldx = D + 5 with NaN in the pad
columns and PAD sentinel elements around every output, the workspace and the stats record.

Bounds of the step.  delta_i = (2 D + 8) 2^-24 (n_i + max_c m_c): the fp32 chain's error in 2 g_ic (D products and D
additions, each 2^-24 relative to at most |x_i| |c| <= (n_i + m_c) / 2, doubled) and the roundings of n_i, m_c, their sum
and the difference.
  |dist2 - d2_64| <= delta_i; labels equal wherever the restatement's lead (second-best minus best) exceeds 2 delta_i; at
  most 1 % of the rows may be left out (asserted).
  counts: exact for the device's own labels.  new_centroids: against the fp64 mean over the device's labels, within
  2^-17 max_i |x_id| per column (63 fp32 additions of a tile partial, each 2^-24 of a partial <= 64 max |x|, and the
  store).  inertia: the fp64 sum of the device's dist2 to 1e-12 relative; shift2 likewise from the stored centroids;
  changed and empty exactly.  A second call with ldx = D gives the same bits.

Seeding: mind2[row] == 0 exactly, also for a planted copy of the row; |e - e64| <= (D + 4) 2^-24 e64 (D products and D
additions of non-negative terms, the differences' roundings).

Fit: on well-separated clusters the restatement must reach ARI 1 with every lead above 2 delta; the device fit then has
the same labels and iteration count.
"""
import functools
import struct

import numpy as np
import pandas as pd
import pytest
import torch

from tests import kmeans_restatement as K
from tests import sil_restatement as R

pytestmark = pytest.mark.gpu

PAD = 8
SHAPES = [(5, 3, 2), (70, 8, 3), (300, 70, 5), (1030, 130, 7), (200, 512, 4), (600, 16, 256), (2100, 128, 37)]


def make_case(N, D, C):
    seed = 1000 * D + N
    X, _ = R.clusters(seed, N, D, min(C, 8))
    X32 = (X - X.mean(0, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    cen = X32[rng.choice(N, C, replace=False)] + (0.3 * rng.standard_normal((C, D))).astype(np.float32)
    return X32, cen.astype(np.float32)


def delta_of(X, cen):
    X, cen = X.astype(np.float64), np.asarray(cen, dtype=np.float64)
    return (2 * X.shape[1] + 8) * 2.0 ** -24 * ((X * X).sum(1) + (cen * cen).sum(1).max())


@functools.lru_cache(maxsize=None)
def reference(N, D, C):
    """Inputs and the restatement's step of one shape; computed once and never written to."""
    X, cen = make_case(N, D, C)
    out = K.step(X, cen)
    out.update(X=X, cen=cen, delta=delta_of(X, cen))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _lib():
    from mmvae_amd import _clust_lib

    return _clust_lib, _clust_lib.load_clust()


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


def wide_rows(X, extra_ld):
    N, D = X.shape
    wide = torch.full((N, D + extra_ld), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :D] = torch.from_numpy(np.array(X)).cuda()
    return wide


def run_step(X, cen, label_in=None, extra_ld=5):
    """The C entry on rows with leading dimension D + extra_ld (NaN in the pad columns), into sentinel-padded outputs, a
    stats record between sentinel bytes and a workspace of exactly the asked size followed by sentinel bytes."""
    L, lib = _lib()
    N, D = X.shape
    C = len(cen)
    wide = wide_rows(X, extra_ld)
    cen_d = torch.from_numpy(np.array(cen)).cuda()
    new = Padded(C * D, torch.float32, -5.0)
    label = Padded(N, torch.int32, -99)
    label.body[:] = -1 if label_in is None else torch.from_numpy(np.array(label_in, dtype=np.int32)).cuda()
    dist2 = Padded(N, torch.float32, -5.0)
    counts = Padded(C, torch.int32, -99)
    stats = Padded(24, torch.uint8, 0xCD)  # (PAD = 8 bytes in front: the record is 8-byte aligned)
    nbytes = lib.mmvae_clust_kmeans_workspace_bytes(N, D, C)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    L.check(lib.mmvae_clust_kmeans_step_f32(N, D, wide.data_ptr(), D + extra_ld, C, cen_d.data_ptr(), new.ptr(), label.ptr(),
                                            dist2.ptr(), counts.ptr(), stats.ptr(), ws.data_ptr(), nbytes, _stream()),
            "mmvae_clust_kmeans_step_f32")
    torch.cuda.synchronize()
    for name, buf in (("new_centroids", new), ("label", label), ("dist2", dist2), ("counts", counts), ("stats", stats)):
        assert buf.untouched_outside(), f"{name}: written outside its elements"
    assert bool((ws[nbytes:] == 0xAB).all()), "written past the workspace"
    inertia, shift2, changed, empty = struct.unpack("<ddii", bytes(stats.body.cpu().numpy()))
    return dict(new=new.body.cpu().numpy().reshape(C, D), label=label.body.cpu().numpy(), dist2=dist2.body.cpu().numpy(),
                counts=counts.body.cpu().numpy(), inertia=inertia, shift2=shift2, changed=changed, empty=empty)


def check_outputs_against_themselves(got, X, cen, label_in=None):
    """counts, new_centroids, inertia, shift2, changed and empty from the device's own labels and dist2."""
    N, D = X.shape
    C = len(cen)
    X64, cen64 = X.astype(np.float64), cen.astype(np.float64)
    assert got["label"].min() >= 0 and got["label"].max() < C
    counts = np.bincount(got["label"], minlength=C)
    assert np.array_equal(got["counts"], counts)
    tol = 2.0 ** -17 * np.abs(X64).max(0)
    for c in range(C):
        if counts[c] == 0:
            assert np.array_equal(got["new"][c].view(np.uint32), cen[c].view(np.uint32)), f"empty cluster {c} moved"
        else:
            assert (np.abs(got["new"][c] - X64[got["label"] == c].mean(0)) <= tol).all(), f"cluster {c}"
    inertia = got["dist2"].astype(np.float64).sum()
    assert abs(got["inertia"] - inertia) <= 1e-12 * inertia
    shift2 = ((got["new"].astype(np.float64) - cen64) ** 2).sum()
    assert abs(got["shift2"] - shift2) <= 1e-12 * shift2
    old = np.full(N, -1) if label_in is None else np.asarray(label_in)
    assert got["changed"] == int((got["label"] != old).sum()) and got["empty"] == int((counts == 0).sum())


@pytest.mark.parametrize("N, D, C", SHAPES)
def test_step_matches_the_restatement(N, D, C):
    ref = reference(N, D, C)
    X, cen, delta = ref["X"], ref["cen"], ref["delta"]
    got = run_step(X, cen)
    err = np.abs(got["dist2"] - ref["d2"])
    sure = ref["lead"] > 2 * delta
    print(f"N={N} D={D} C={C}: |dist2 - d2_64| / delta max {np.max(err / delta):.3f}, unsure rows {(~sure).sum()} "
          f"({100 * (~sure).mean():.2f} %), mismatches among them {(got['label'] != ref['label']).sum()}")
    assert (~sure).mean() <= 0.01, f"{(~sure).sum()} rows are not sure of their cluster"
    assert (err <= delta).all()
    assert np.array_equal(got["label"][sure], ref["label"][sure])
    check_outputs_against_themselves(got, X, cen)
    assert got["changed"] == N
    again = run_step(X, cen, extra_ld=0)
    for name in ("new", "label", "dist2", "counts"):
        assert np.array_equal(again[name], got[name]), name
    assert all(again[k] == got[k] for k in ("inertia", "shift2", "changed", "empty"))


def test_planted_empty_clusters_and_preset_labels():
    N, D, C = 300, 70, 5
    ref = reference(N, D, C)
    X = ref["X"]
    cen = np.array(ref["cen"])
    cen[4] = cen[1]        # two bit-equal centroids: every tie goes to the smaller index
    cen[2] = 1.0e3         # far from every row
    want = K.step(X, cen)
    assert want["counts"][1] > 0 and want["counts"][4] == 0 and want["counts"][2] == 0
    got = run_step(X, cen)
    check_outputs_against_themselves(got, X, cen)
    assert got["counts"][4] == 0 and got["counts"][2] == 0 and got["counts"][1] > 0 and got["empty"] == 2
    assert np.array_equal(got["new"][4].view(np.uint32), cen[4].view(np.uint32))
    assert np.array_equal(got["new"][2].view(np.uint32), cen[2].view(np.uint32))
    # the restatement's labels as the labels of the iteration before: only rows it is not sure of may change
    cen = ref["cen"]
    sure = ref["lead"] > 2 * ref["delta"]
    preset = run_step(X, cen, label_in=ref["label"])
    mismatch = preset["label"] != ref["label"]
    assert preset["changed"] == int(mismatch.sum()) and not mismatch[sure].any()
    check_outputs_against_themselves(preset, X, cen, ref["label"])
    first = run_step(X, cen)
    assert np.array_equal(first["label"], preset["label"]) and np.array_equal(first["new"], preset["new"])


def run_seed(X, row, first, mind2_in=None, extra_ld=5):
    L, lib = _lib()
    N, D = X.shape
    wide = wide_rows(X, extra_ld)
    mind2 = Padded(N, torch.float32, -5.0)
    if mind2_in is not None:
        mind2.body[:] = torch.from_numpy(mind2_in).cuda()
    L.check(lib.mmvae_clust_seed_update_f32(N, D, wide.data_ptr(), D + extra_ld, row, first, mind2.ptr(), _stream()),
            "mmvae_clust_seed_update_f32")
    torch.cuda.synchronize()
    assert mind2.untouched_outside(), "mind2: written outside its rows"
    return mind2.body.cpu().numpy()


@pytest.mark.parametrize("N, D, C", SHAPES)
def test_seed_update_matches_the_direct_form(N, D, C):
    X = np.array(reference(N, D, C)["X"])
    row, copy = N // 3, N - 1
    X[copy] = X[row]
    X64 = X.astype(np.float64)
    e64 = ((X64 - X64[row]) ** 2).sum(1)
    got = run_seed(X, row, 1)
    assert got[row] == 0 and got[copy] == 0
    assert (np.abs(got - e64) <= (D + 4) * 2.0 ** -24 * e64).all()
    other = 0
    f64 = ((X64 - X64[other]) ** 2).sum(1)
    both = run_seed(X, other, 0, got)
    direct = run_seed(X, other, 1, extra_ld=0)
    assert (np.abs(direct - f64) <= (D + 4) * 2.0 ** -24 * f64).all() and direct[other] == 0
    assert np.array_equal(both, np.minimum(got, direct))


def sure_uniforms(X, C, seed):
    """C uniforms whose every threshold lies more than 1e-5 of the total from an edge of the cumulative sum."""
    for trial in range(20):
        u = np.random.default_rng(seed + trial).random(C)
        rows, margin = K.seed(X, C, u)
        if margin > 1e-5:
            return u, rows, margin
    raise AssertionError("no uniforms with a safe margin")


@pytest.mark.parametrize("N, D, C", [(300, 70, 5), (2100, 128, 37)])
def test_kmeans_seed_returns_the_restatement_rows(N, D, C):
    from mmvae_amd import clustering

    X = reference(N, D, C)["X"]
    u, rows, margin = sure_uniforms(X, C, 7)
    assert margin > 1e-5 and len(set(rows.tolist())) == C
    got = clustering.kmeans_seed(torch.from_numpy(np.array(X)).cuda(), C, u)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), rows)


def separate_clusters(N, D, C, spread=0.05, centre_scale=3.0):
    X, which = R.clusters(50 * D + N, N, D, C, spread=spread, centre_scale=centre_scale)
    return X.astype(np.float32), which


@functools.lru_cache(maxsize=None)
def reference_fit(N, D, C, spread, centre_scale):
    X, which = separate_clusters(N, D, C, spread, centre_scale)
    want = K.fit(X, C, seed_value=0, round32=True)
    n = (want["Xc"] ** 2).sum(1)
    want.update(X=X, which=which, delta=(2 * D + 8) * 2.0 ** -24 * (n + n.max()))
    return want


def check_fit_invariants(fit, x, N, C, delta_sum):
    from mmvae_amd import clustering

    assert fit.labels.dtype == torch.int32 and fit.labels.is_cuda and fit.labels.shape == (N,)
    assert fit.centroids.shape == fit.centred.shape == (C, x.shape[1]) and fit.centroids.dtype == torch.float32
    assert int(fit.counts.sum()) == N and len(fit.history) == fit.n_iter
    assert np.array_equal(fit.counts.cpu().numpy(), np.bincount(fit.labels.cpu().numpy(), minlength=C))
    assert all(b <= a + delta_sum for a, b in zip(fit.history, fit.history[1:])), fit.history
    xc = (x.double() - fit.offset).float()
    new, label, dist2, counts, stats = clustering.kmeans_step(xc, fit.centred, fit.labels)
    assert stats.changed == 0 and torch.equal(label, fit.labels) and stats.inertia == fit.inertia
    again = clustering.kmeans_fit(x, C)
    assert torch.equal(again.labels, fit.labels) and torch.equal(again.centroids, fit.centroids)
    assert again.inertia == fit.inertia and again.history == fit.history and again.n_iter == fit.n_iter
    return stats


@pytest.mark.parametrize("N, D, C", [(1030, 130, 7), (2100, 128, 37)])
def test_fit_on_separate_clusters_equals_the_restatement(N, D, C):
    from mmvae_amd import clustering

    want = reference_fit(N, D, C, 0.05, 3.0)
    assert K.ari(want["labels"], want["which"]) == 1.0 and want["converged"]
    assert want["min_lead"] > 2 * want["delta"].max(), (want["min_lead"], want["delta"].max())
    x = torch.from_numpy(want["X"]).cuda()
    fit = clustering.kmeans_fit(x, C)
    assert np.array_equal(fit.labels.cpu().numpy(), want["labels"]) and fit.n_iter == want["n_iter"] and fit.converged
    assert abs(fit.inertia - want["inertia"]) <= want["delta"].sum()
    scale = np.abs(want["X"]).max()
    assert np.abs(fit.centroids.cpu().numpy() - want["centroids"]).max() <= 2.0 ** -16 * scale
    stats = check_fit_invariants(fit, x, N, C, want["delta"].sum())
    assert stats.shift2 == 0.0 and stats.empty == 0
    table = clustering.contingency(fit.labels, torch.from_numpy(want["which"]).cuda())
    assert clustering.adjusted_rand_index(table) == 1.0 and abs(clustering.normalized_mutual_info(table) - 1.0) <= 1e-12


def test_fit_on_overlapping_clusters_keeps_its_invariants():
    from mmvae_amd import clustering

    N, D, C = 1030, 130, 7
    X, which = separate_clusters(N, D, C, spread=3.0, centre_scale=1.0)
    Xc = K.centred(X, True)
    n = (Xc ** 2).sum(1)
    delta_sum = ((2 * D + 8) * 2.0 ** -24 * (n + n.max())).sum()
    x = torch.from_numpy(X).cuda()
    fit = clustering.kmeans_fit(x, C)
    check_fit_invariants(fit, x, N, C, delta_sum)
    assert 1 <= fit.n_iter <= 300 and (fit.converged or fit.n_iter == 300)
    table = clustering.contingency(fit.labels, torch.from_numpy(which).cuda(), C, C)
    nmi, ari = clustering.normalized_mutual_info(table), clustering.adjusted_rand_index(table)
    print(f"overlapping clusters: n_iter {fit.n_iter}, converged {fit.converged}, nmi {nmi:.4f}, ari {ari:.4f}")
    assert 0.0 <= nmi <= 1.0 and 0.0 <= ari <= 1.0


def test_refusals_leave_the_outputs_untouched():
    L, lib = _lib()
    N, D, C = 40, 6, 3
    x = torch.zeros((N, D), dtype=torch.float32, device="cuda")
    cen = torch.zeros((C, D), dtype=torch.float32, device="cuda")
    new = Padded(C * D, torch.float32, -5.0)
    label = Padded(N, torch.int32, -99)
    dist2 = Padded(N, torch.float32, -5.0)
    counts = Padded(C, torch.int32, -99)
    stats = Padded(24, torch.uint8, 0xCD)
    nbytes = lib.mmvae_clust_kmeans_workspace_bytes(N, D, C)
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    ok = [N, D, x.data_ptr(), D, C, cen.data_ptr(), new.ptr(), label.ptr(), dist2.ptr(), counts.ptr(), stats.ptr(),
          ws.data_ptr(), nbytes, _stream()]
    bad = [{0: 0}, {0: 2}, {1: 0}, {1: 513}, {3: D - 1}, {4: 0}, {4: N + 1}, {4: 257}, {12: nbytes - 1},
           {11: ws.data_ptr() + 4}, {10: stats.ptr() + 4}] + [{i: None} for i in (2, 5, 6, 7, 8, 9, 10, 11)]
    refused = [lib.mmvae_clust_kmeans_step_f32(*[change.get(i, v) for i, v in enumerate(ok)]) for change in bad]
    mind2 = Padded(N, torch.float32, -5.0)
    ok = [N, D, x.data_ptr(), D, 3, 1, mind2.ptr(), _stream()]
    bad_seed = [{0: 0}, {1: 0}, {1: 513}, {3: D - 1}, {4: -1}, {4: N}, {2: None}, {6: None}]
    refused_seed = [lib.mmvae_clust_seed_update_f32(*[change.get(i, v) for i, v in enumerate(ok)]) for change in bad_seed]
    torch.cuda.synchronize()
    assert refused == [L.ERR_ARG] * len(bad), refused
    assert refused_seed == [L.ERR_ARG] * len(bad_seed), refused_seed
    for name, buf in (("new", new), ("label", label), ("dist2", dist2), ("counts", counts), ("stats", stats), ("mind2", mind2)):
        assert buf.untouched(), name
    assert bool((ws == 0xAB).all())


def test_cluster_metrics_tables_equal_the_restatement():
    from mmvae_amd import clustering

    X, cluster = R.clusters(31, 240, 12, 3, spread=0.3)
    X32 = X.astype(np.float32)
    meta = pd.DataFrame({"cell_type": np.array(["B", "NK", "T"], dtype=object)[cluster],
                         "tissue": np.where(np.arange(240) % 2 == 0, "gut", "lung")})
    meta.loc[5, "cell_type"] = np.nan
    label = pd.factorize(meta["cell_type"], sort=True)[0].astype(np.int32)
    tissue = pd.factorize(meta["tissue"], sort=True)[0].astype(np.int32)
    out = clustering.cluster_metrics(torch.from_numpy(X32).cuda(), meta, ("cell_type", "tissue"), seed=3)
    assert out.columns == ("cell_type", "tissue") and np.array_equal(out.codes.cpu().numpy(), np.stack([label, tissue]))
    assert tuple(out.summary.columns) == clustering.SUMMARY_COLUMNS and label[5] == -1
    assert out.summary["n_clusters"].tolist() == [3, 2] and out.summary["n_cells"].tolist() == [239, 240]
    for n, (key, C, codes) in enumerate((("cell_type", 3, label), ("tissue", 2, tissue))):
        want = K.fit(X32, C, seed_value=3, round32=True)
        norms = (want["Xc"] ** 2).sum(1)
        delta = (2 * 12 + 8) * 2.0 ** -24 * (norms + norms.max())
        assert want["min_lead"] > 2 * delta.max() and want["converged"]
        assert np.array_equal(out.fits[key].labels.cpu().numpy(), want["labels"]) and out.summary["n_iter"][n] == want["n_iter"]
        table = out.contingency[key]
        assert np.array_equal(table.values, K.table_of(want["labels"], codes)) and table.columns.tolist() == list(out.categories[key])
        assert abs(out.summary["nmi"][n] - K.nmi(want["labels"], codes)) <= 1e-12
        assert abs(out.summary["ari"][n] - K.ari(want["labels"], codes)) <= 1e-12
        assert abs(out.summary["inertia"][n] - want["inertia"]) <= delta.sum() and bool(out.summary["converged"][n])
    assert out.summary["ari"][0] == 1.0 and out.summary["ari"][1] < 0.5


def test_trainer_cluster_metrics_on_the_smallest_golden_case(tmp_path, monkeypatch):
    from mmvae_amd import clustering
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
    monkeypatch.setattr(trainer, "predict", lambda m, b: predictions)  # the same latent samples for both calls below
    out = trainer.cluster_metrics(model, batches, label_keys=("group",))
    assert isinstance(out, clustering.ClusterMetrics) and out.codes.shape == (1, 2 * B)
    fit = out.fits["group"]
    assert fit.labels.is_cuda and fit.labels.shape == (2 * B,) and int(fit.counts.sum()) == 2 * B
    assert np.isfinite(out.summary[["nmi", "ari", "inertia"]].values.astype(float)).all()
    assert out.summary["n_clusters"].tolist() == [2] and out.summary["n_cells"].tolist() == [2 * B]
    outs = [p[RK.Z] for p in predictions]
    direct = clustering.cluster_metrics(torch.cat([o[0] for o in outs], 0),
                                        pd.concat([o[1] for o in outs], ignore_index=True), ("group",))
    assert direct.summary.equals(out.summary) and direct.contingency["group"].equals(out.contingency["group"])
    assert torch.equal(direct.fits["group"].labels, fit.labels)
