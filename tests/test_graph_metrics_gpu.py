"""GPU checks of libmmvae_graph.so (include/mmvae_graph.h) and mmvae_amd.graph_metrics against the independent numpy
restatement (tests/graph_restatement.py).  The tables come from the restatement's side (hand-made, random, or its own
brute-force kNN): the kNN kernel is not under test here, except in the end-to-end test, where the restatement reads the
graph the device made.

Bounds.  Roots, counts, sizes and component numbers are integers: equal, and equal bits on a second call.  stat is held
to (B + 3) 2^-53 stat (three roundings per term and a sum of non-negative terms); it has been bit-equal on every case.
pval, where the restatement's p >= 1e-290: P_REL relative, the next power of two above four times the largest deviation
measured over these cases (P_MEASURED; profiles/graph.txt); below 1e-290 only 0 <= p <= 1e-280.  A rejection p < alpha
must agree wherever the restatement's p is not within 1e-9 alpha of alpha, and at most 1 % of the rows may be that close.
"""
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch

from tests import graph_restatement as R

pytestmark = pytest.mark.gpu

P_MEASURED = 4.108e-14   # the "64 batches" rows; the kNN cases 5.8e-15, 1.1e-15 and 1.4e-14
P_REL = 2.0 ** -42       # 2.27e-13 > 4 * 4.108e-14 = 1.64e-13 > 2^-43
ALPHA = 0.05
PAD = 8  # sentinel elements in front of and behind every output

KNN_COMPONENT_CASES = {"knn 600": (600, 16, 8, 5, 2.0), "knn 4096": (4096, 8, 4, 3, 1.0)}
KBET_CASES = [(600, 16, 16, 2), (2000, 32, 31, 3), (1500, 8, 64, 7)]
HAND_NAMES = ["path", "path permuted", "ring", "star", "all self", "one vertex", "257 x 3", "duplicates and selves",
              "cliques, one code", "cliques, two codes", "cliques, one end unlabelled", "cliques, no codes"]
COMPONENT_NAMES = HAND_NAMES + list(KNN_COMPONENT_CASES) + ["random 200000 x 8"]


@functools.lru_cache(maxsize=None)
def _hand_tables():
    return R.hand_tables()


@functools.lru_cache(maxsize=None)
def component_reference(name):
    """Inputs and the restatement's results of one case; computed once and never written to."""
    if name in KNN_COMPONENT_CASES:
        idx, codes, n_classes = R.knn_component_case(*KNN_COMPONENT_CASES[name])
    elif name.startswith("random"):
        idx, codes, n_classes = R.random_table(200_000, 8), None, 1
    else:
        idx, codes, n_classes = _hand_tables()[name]
    root = R.components(idx, codes)
    count, largest, n_comp = R.component_sizes(root, codes, n_classes)
    for a in (idx, codes, root, count, largest):
        if a is not None:
            a.setflags(write=False)
    return dict(idx=idx, codes=codes, n_classes=n_classes, root=root, count=count, largest=largest, n_comp=n_comp)


@functools.lru_cache(maxsize=None)
def kbet_reference(name):
    if isinstance(name, tuple):
        idx, batch = R.kbet_case(*name)
        freq, n_batches = None, name[3]
    else:
        idx, batch, freq, n_batches = R.kbet_hand_cases()[name]
    stat, pval = R.kbet(idx, batch, n_batches, freq)
    for a in (idx, batch, stat, pval):
        a.setflags(write=False)
    return dict(idx=idx, batch=batch, freq=freq, n_batches=n_batches, stat=stat, pval=pval)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # a copy: the references are read-only


def _lib():
    from mmvae_amd import _graph_lib

    return _graph_lib, _graph_lib.load_graph()


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


# ------------------------------------------------------------------------------------------------ connected components
@pytest.mark.parametrize("name", COMPONENT_NAMES)
def test_components_equal_the_restatement(name):
    from mmvae_amd import graph_metrics as G

    ref = component_reference(name)
    idx, codes = _dev(ref["idx"]), _dev(ref["codes"])
    root, rounds = G.connected_components(idx, codes)
    again, rounds_again = G.connected_components(idx, codes)
    print(f"{name}: N = {idx.shape[0]}, k = {idx.shape[1]}, rounds {rounds} and {rounds_again}, "
          f"{ref['n_comp']} components, largest {ref['largest'].tolist()} of {ref['count'].tolist()}")
    assert root.dtype == torch.int32 and root.is_cuda
    assert np.array_equal(root.cpu().numpy(), ref["root"])
    assert 1 <= rounds <= G.MAX_ROUNDS and 1 <= rounds_again <= G.MAX_ROUNDS
    assert torch.equal(root, again)
    count, largest, n_comp = G.component_sizes(root, codes, ref["n_classes"])
    assert count.dtype == torch.int64 and largest.dtype == torch.int32
    assert np.array_equal(count.cpu().numpy(), ref["count"]) and np.array_equal(largest.cpu().numpy(), ref["largest"])
    assert n_comp == ref["n_comp"]
    if ref["codes"] is not None:
        conn = G.graph_connectivity(idx, codes, ref["n_classes"])
        per, mean, _ = R.connectivity(ref["idx"], ref["codes"], ref["n_classes"])
        assert np.array_equal(conn.per_class.cpu().numpy(), per, equal_nan=True) and conn.score == mean
        assert torch.equal(conn.root, root) and conn.n_components == n_comp


def test_the_cases_say_what_they_are_meant_to():
    ref = component_reference("knn 4096")
    per = ref["largest"] / ref["count"]
    assert (per < 1.0).any() and (per > 0.5).all(), per       # a class that is not in one piece
    assert (ref["codes"] < 0).mean() > 0.01
    merged, apart, gap = (component_reference(f"cliques, {v}") for v in ("one code", "two codes", "one end unlabelled"))
    assert (merged["largest"].tolist(), merged["n_comp"]) == ([64], 1)
    assert (apart["largest"].tolist(), apart["n_comp"]) == ([32, 32], 2)
    assert (gap["count"].tolist(), gap["largest"].tolist(), gap["n_comp"], int(gap["root"][32])) == ([63], [32], 2, 32)
    assert component_reference("all self")["n_comp"] == 130 and component_reference("star")["n_comp"] == 1
    assert component_reference("path permuted")["n_comp"] == 1 and component_reference("one vertex")["n_comp"] == 1


def test_round_entry_writes_inside_its_rows_and_max_rounds_is_kept():
    from mmvae_amd import graph_metrics as G

    L, lib = _lib()
    ref = component_reference("257 x 3")
    idx, codes = _dev(ref["idx"]), _dev(ref["codes"])
    N, k = idx.shape
    parent, changed = Padded(N, torch.int32, -77), Padded(1, torch.int32, -77)
    parent.body.copy_(torch.arange(N, dtype=torch.int32))
    for rounds in range(1, G.MAX_ROUNDS + 1):
        changed.body.zero_()
        L.check(lib.mmvae_graph_cc_round_i32(N, k, idx.data_ptr(), codes.data_ptr(), parent.ptr(), changed.ptr(), _stream()),
                "cc_round")
        if int(changed.body) == 0:
            break
    assert np.array_equal(parent.body.cpu().numpy(), ref["root"]) and rounds > 1
    assert parent.untouched_outside() and changed.untouched_outside()
    size_ws, count = Padded(N, torch.int32, -77), Padded(2, torch.int64, -77)
    largest, n_comp = Padded(2, torch.int32, -77), Padded(1, torch.int32, -77)
    L.check(lib.mmvae_graph_component_sizes_i32(N, parent.ptr(), codes.data_ptr(), 2, size_ws.ptr(), count.ptr(),
                                                largest.ptr(), n_comp.ptr(), _stream()), "component_sizes")
    torch.cuda.synchronize()
    for name, buf in (("size_ws", size_ws), ("count", count), ("largest", largest), ("n_comp", n_comp)):
        assert buf.untouched_outside(), name
    assert np.array_equal(count.body.cpu().numpy(), ref["count"]) and int(n_comp.body) == ref["n_comp"]
    labelled = ref["codes"] >= 0
    assert np.array_equal(size_ws.body.cpu().numpy(), np.bincount(ref["root"][labelled], minlength=N))
    path = _dev(component_reference("path")["idx"])
    with pytest.raises(RuntimeError, match="max_rounds = 1"):
        G.connected_components(path, max_rounds=1)
    wild = idx.clone()
    wild[5, 1] = N
    with pytest.raises(ValueError, match="neighbour indices"):
        G.connected_components(wild)
    with pytest.raises(ValueError, match="int32"):
        G.connected_components(idx.long())


# ---------------------------------------------------------------------------------------------------------------- kBET
def run_kbet(ref):
    """stat and pval of one case through the C entry, into sentinel-padded outputs."""
    L, lib = _lib()
    idx, batch = _dev(ref["idx"]), _dev(ref["batch"])
    N, k = idx.shape
    freq = R.batch_frequencies(ref["batch"], ref["n_batches"]) if ref["freq"] is None else ref["freq"]
    dof = int((freq > 0).sum()) - 1
    stat, pval = Padded(N, torch.float64, -7.0), Padded(N, torch.float64, -7.0)
    L.check(lib.mmvae_graph_kbet_f64(N, k, idx.data_ptr(), batch.data_ptr(), ref["n_batches"], _dev(freq).data_ptr(), dof,
                                     stat.ptr(), pval.ptr(), _stream()), "kbet")
    torch.cuda.synchronize()
    assert stat.untouched_outside() and pval.untouched_outside()
    return stat.body.cpu().numpy(), pval.body.cpu().numpy()


def check_kbet(name, ref, got_stat, got_p):
    stat, pval, B = ref["stat"], ref["pval"], ref["n_batches"]
    nan = np.isnan(stat)
    assert np.array_equal(np.isnan(got_stat), nan) and np.array_equal(np.isnan(got_p), nan), name
    ok = ~nan
    stat_dev = np.abs(got_stat[ok] - stat[ok])
    big = ok & (pval >= 1e-290)
    rel = np.abs(got_p[big] - pval[big]) / pval[big]
    close = np.abs(pval - ALPHA) <= 1e-9 * ALPHA
    print(f"{name}: {int(ok.sum())} rows, stat bit-equal on {np.mean(got_stat[ok] == stat[ok]):.4f} "
          f"(largest deviation {stat_dev.max() if ok.any() else 0.0:.3e}), p relative deviation at most "
          f"{rel.max() if big.any() else 0.0:.3e} on {int(big.sum())} rows, {int(close.sum())} rows within the margin of alpha, "
          f"rejection rate {R.rejection_rate(pval, ALPHA):.4f}, p from {np.nanmin(pval):.3e}")
    assert (stat_dev <= (B + 3) * 2.0 ** -53 * stat[ok]).all(), name
    assert (rel <= P_REL).all(), (name, rel.max())
    small = ok & ~big
    assert ((got_p[small] >= 0.0) & (got_p[small] <= 1e-280)).all(), name
    assert ((got_p[ok] >= 0.0) & (got_p[ok] <= 1.0)).all() and (got_p[ok & (stat == 0.0)] == 1.0).all(), name
    assert close.mean() <= 0.01, name
    firm = ok & ~close
    assert np.array_equal(got_p[firm] < ALPHA, pval[firm] < ALPHA), name
    return rel.max() if big.any() else 0.0


@pytest.mark.parametrize("shape", KBET_CASES)
def test_kbet_on_knn_graphs_matches_the_restatement(shape):
    from mmvae_amd import graph_metrics as G

    ref = kbet_reference(shape)
    rate = R.rejection_rate(ref["pval"], ALPHA)
    assert 0.2 < rate < 0.995, rate                      # neither outcome is trivial
    assert (ref["batch"] < 0).any() and len(set(np.bincount(ref["batch"][ref["batch"] >= 0]))) == shape[3]
    got_stat, got_p = run_kbet(ref)
    check_kbet(str(shape), ref, got_stat, got_p)
    # the python entry: the same bits, the global frequencies by default, and the rate of the restatement
    stat, pval, rejection = G.kbet(_dev(ref["idx"]), _dev(ref["batch"]), alpha=ALPHA)
    assert np.array_equal(stat.cpu().numpy(), got_stat, equal_nan=True)
    assert np.array_equal(pval.cpu().numpy(), got_p, equal_nan=True)
    assert rejection == rate
    again = G.kbet(_dev(ref["idx"]), _dev(ref["batch"]), torch.from_numpy(R.batch_frequencies(ref["batch"], shape[3])))
    assert torch.equal(again[1].nan_to_num(-1.0), pval.nan_to_num(-1.0))


@pytest.mark.parametrize("name", ["two batches", "a batch of share 0", "k = 2", "a rare batch", "64 batches"])
def test_kbet_on_hand_made_rows(name):
    ref = kbet_reference(name)
    got_stat, got_p = run_kbet(ref)
    check_kbet(name, ref, got_stat, got_p)
    if name == "two batches":
        assert got_stat[0] == 4.0 == got_stat[3] and (got_stat[1], got_p[1]) == (0.0, 1.0)   # one batch only; at expectation
        assert math.isnan(got_stat[2]) and math.isnan(got_p[2])                              # nobody labelled
        assert got_stat[4] == 0.0                                                            # k_i = 2: one and one
    if name == "a rare batch":
        assert (ref["pval"] < 1e-290).all() and (got_stat > 1e5).all()


def test_refusals_leave_the_outputs_untouched():
    L, lib = _lib()
    N, k = 40, 8
    idx = torch.zeros((N, 65), dtype=torch.int32, device="cuda")
    codes = torch.zeros(N, dtype=torch.int32, device="cuda")
    freq = torch.full((3,), 1 / 3, dtype=torch.float64, device="cuda")
    parent, changed = Padded(N, torch.int32, -77), Padded(1, torch.int32, -77)
    size_ws, count = Padded(N, torch.int32, -77), Padded(3, torch.int64, -77)
    largest, n_comp = Padded(3, torch.int32, -77), Padded(1, torch.int32, -77)
    stat, pval = Padded(N, torch.float64, -7.0), Padded(N, torch.float64, -7.0)
    s = _stream()
    i, c, f = idx.data_ptr(), codes.data_ptr(), freq.data_ptr()
    cc = lambda *a: lib.mmvae_graph_cc_round_i32(*a, s)  # noqa: E731
    refused = [cc(0, k, i, c, parent.ptr(), changed.ptr()), cc(N, 0, i, c, parent.ptr(), changed.ptr()),
               cc(N, 65, i, c, parent.ptr(), changed.ptr()), cc(N, k, None, c, parent.ptr(), changed.ptr()),
               cc(N, k, i, c, None, changed.ptr()), cc(N, k, i, c, parent.ptr(), None)]
    sz = lambda *a: lib.mmvae_graph_component_sizes_i32(*a, s)  # noqa: E731
    outs = (size_ws.ptr(), count.ptr(), largest.ptr(), n_comp.ptr())
    refused += [sz(0, c, c, 3, *outs), sz(N, None, c, 3, *outs), sz(N, c, c, 0, *outs), sz(N, c, None, 3, *outs)]
    refused += [sz(N, c, c, 3, *[None if n == m else p for n, p in enumerate(outs)]) for m in range(4)]
    kb = lambda *a: lib.mmvae_graph_kbet_f64(*a, s)  # noqa: E731
    refused += [kb(0, k, i, c, 3, f, 2, stat.ptr(), pval.ptr()), kb(N, 1, i, c, 3, f, 2, stat.ptr(), pval.ptr()),
                kb(N, 65, i, c, 3, f, 2, stat.ptr(), pval.ptr()), kb(N, k, i, c, 1, f, 1, stat.ptr(), pval.ptr()),
                kb(N, k, i, c, 65, f, 2, stat.ptr(), pval.ptr()), kb(N, k, i, c, 3, f, 0, stat.ptr(), pval.ptr()),
                kb(N, k, i, c, 3, f, 3, stat.ptr(), pval.ptr()), kb(N, k, None, c, 3, f, 2, stat.ptr(), pval.ptr()),
                kb(N, k, i, None, 3, f, 2, stat.ptr(), pval.ptr()), kb(N, k, i, c, 3, None, 2, stat.ptr(), pval.ptr()),
                kb(N, k, i, c, 3, f, 2, None, pval.ptr()), kb(N, k, i, c, 3, f, 2, stat.ptr(), None)]
    torch.cuda.synchronize()
    assert refused == [L.ERR_ARG] * len(refused), refused
    for name, buf in (("parent", parent), ("changed", changed), ("size_ws", size_ws), ("count", count),
                      ("largest", largest), ("n_comp", n_comp), ("stat", stat), ("pval", pval)):
        assert buf.untouched(), name


# ---------------------------------------------------------------------------------------------------------- end to end
def test_graph_metrics_end_to_end_against_the_restatement():
    from mmvae_amd import graph_metrics as G
    from mmvae_amd.umap import knn_graph

    N = 2000
    X, cluster = R.mixture(31, N, 32, 4, scale=1.0)
    rng = np.random.default_rng(32)
    batch = (rng.random(N) < 0.35).astype(np.int32)
    X = X + 0.5 * rng.standard_normal((2, 32)).astype(np.float32)[batch]
    coarse = np.where(cluster < 2, "lymphoid", "myeloid").astype(object)
    coarse[rng.random(N) < 0.02] = np.nan
    meta = pd.DataFrame({"species": np.where(batch == 0, "human", "mouse"), "cell_type": [f"t{c}" for c in cluster],
                         "lineage": coarse})
    z = torch.from_numpy(X).cuda()
    out = G.graph_metrics(z, meta, label_keys=("cell_type", "lineage"), n_neighbors=6)
    assert out.idx.shape == (N, 6) and out.idx.is_cuda and out.kbet_pval.is_cuda
    assert tuple(out.summary.columns) == G.SUMMARY_COLUMNS and out.summary["column"].tolist() == ["cell_type", "lineage"]
    idx = out.idx.cpu().numpy()  # the restatement runs on the kernel's own graph
    codes = out.codes.cpu().numpy()
    assert np.array_equal(codes[0], batch) and np.array_equal(codes[1], cluster) and (codes[2] < 0).sum() > 10
    stat, pval = R.kbet(idx, codes[0], 2)
    assert np.array_equal(out.kbet_stat.cpu().numpy(), stat)
    assert (np.abs(out.kbet_pval.cpu().numpy() - pval) <= P_REL * pval).all()
    global_rate = R.rejection_rate(pval, ALPHA)
    for n, (key, L) in enumerate((("cell_type", 4), ("lineage", 2)), start=1):
        row, table = out.summary.iloc[n - 1], out.per_class[key]
        per, mean, n_comp = R.connectivity(idx, codes[n], L)
        assert np.array_equal(out.root[key].cpu().numpy(), R.components(idx, codes[n]))
        assert table["connectivity"].tolist() == per.tolist() and row["graph_connectivity"] == pytest.approx(mean, rel=1e-15)
        assert (row["n_classes"], row["n_cells"], row["n_components"]) == (L, int((codes[n] >= 0).sum()), n_comp)
        assert 1 <= row["cc_rounds"] <= G.MAX_ROUNDS and row["kbet_rejection_global"] == global_rate
        rates = []
        for c in range(L):
            rows = np.nonzero(codes[n] == c)[0]
            k0 = R.kbet_k0(codes[0][rows], 2)
            sub = knn_graph(z[torch.from_numpy(rows).cuda()], k0 + 1)[0].cpu().numpy()
            _, p = R.kbet(sub, codes[0][rows], 2, R.batch_frequencies(codes[0][rows], 2))
            assert (np.abs(p - ALPHA) > 1e-9 * ALPHA).all()
            rates.append(R.rejection_rate(p, ALPHA))
            assert table["kbet_k0"][c] == k0 and bool(table["kbet_tested"][c])
        assert table["kbet_rejection"].tolist() == rates and row["n_classes_tested"] == L
        assert row["kbet_score"] == pytest.approx(1.0 - sum(rates) / L, rel=1e-15)
    assert out.summary["graph_connectivity"][0] < 1.0 and 0.0 < global_rate < 1.0


def test_trainer_graph_metrics_on_the_smallest_golden_case(tmp_path):
    from mmvae_amd import graph_metrics as G
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
    k = min(6, 2 * B - 1)
    frame = lambda g: pd.DataFrame({"group": [g] * B, "donor": [f"d{i % 2}" for i in range(B)]})  # noqa: E731
    out = Trainer().graph_metrics(model, [(x, frame("a"), eid), (x.flip(0) * 0.5, frame("b"), eid)], batch_key="donor",
                                  label_keys=("group",), n_neighbors=k)
    assert isinstance(out, G.GraphMetrics) and out.idx.shape == (2 * B, k) and out.idx.is_cuda
    assert out.codes.shape == (2, 2 * B) and out.root["group"].shape == (2 * B,) and out.kbet_pval.shape == (2 * B,)
    idx, codes = out.idx.cpu().numpy(), out.codes.cpu().numpy()
    assert np.array_equal(out.root["group"].cpu().numpy(), R.components(idx, codes[1]))
    assert np.array_equal(out.kbet_stat.cpu().numpy(), R.kbet(idx, codes[0], 2)[0], equal_nan=True)
    assert out.summary["n_classes"].tolist() == [2] and out.summary["n_cells"].tolist() == [2 * B]
    assert out.summary["graph_connectivity"][0] == R.connectivity(idx, codes[1], 2)[1]
