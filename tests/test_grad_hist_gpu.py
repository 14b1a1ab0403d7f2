"""libmmvae_hist.so on the GPU: bucket counts against np.histogram of the values copied out (exact equality, fp64), the
moments within the bound of their summation order, bit-identical repeats; and the recording of a training run through
the captured engine -- histograms of the arenas' gradients, their norm against the step's logged norms, no effect on the
run."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

from tests import grad_hist_cases as GC

pytestmark = pytest.mark.gpu

MIN, MAX, NUM, SUM, SQ, NONFIN, BELOW, ABOVE = range(8)


def _on_device(values, offsets, lengths, **kw):
    from mmvae_amd.histogram import segment_histograms

    h = segment_histograms(torch.from_numpy(values).cuda(), offsets, lengths, **kw)
    host = h.cpu()
    return host.counts.numpy(), host.stats.numpy()


def test_edge_neighbours():
    from mmvae_amd.histogram import tensorboard_edges

    e = tensorboard_edges()
    v = GC.edge_neighbour_values(e)
    counts, stats = _on_device(v, [0], [v.size])
    ref_counts, ref_stats = GC.reference(v, [0], [v.size], e)
    assert np.array_equal(counts, ref_counts)
    assert int(stats[0, NONFIN]) == 3 and int(stats[0, BELOW]) == 3 and int(stats[0, ABOVE]) == 3
    assert np.array_equal(stats[:, [MIN, MAX, NUM, NONFIN, BELOW, ABOVE]], ref_stats[:, [MIN, MAX, NUM, NONFIN, BELOW, ABOVE]])
    assert stats[0, NUM] + stats[0, NONFIN] == v.size
    assert counts.sum() == v.size - 3 - 3 - 3
    # single values: 0, -0.0 and the smallest denormal in bucket 774, its negative in 773, NaN / inf / 1e30 nowhere
    singles = np.array([0.0, -0.0, 1e-45, -1e-45, np.nan, np.inf, -np.inf, 1e30], dtype=np.float32)
    c1, s1 = _on_device(singles, list(range(8)), [1] * 8)
    assert [int(np.flatnonzero(r)[0]) if r.any() else None for r in c1] == [774, 774, 774, 773, None, None, None, None]
    assert s1[:, NONFIN].tolist() == [0, 0, 0, 0, 1, 1, 1, 0] and s1[:, ABOVE].tolist() == [0] * 7 + [1]


@pytest.fixture(scope="module")
def geometry():
    from mmvae_amd._hist_lib import HIST_ITEM_ELEMS as C
    from mmvae_amd.histogram import tensorboard_edges

    values, offsets, lengths = GC.geometry_case(C)
    ref = GC.reference(values, offsets, lengths, tensorboard_edges())
    return values, offsets, lengths, ref, _on_device(values, offsets, lengths)


def test_segment_geometry(geometry):
    from mmvae_amd.histogram import tensorboard_edges

    values, offsets, lengths, (ref_counts, ref_stats), (counts, stats) = geometry
    e = tensorboard_edges()
    assert np.array_equal(counts, ref_counts)
    sentinel_bucket = int(np.searchsorted(e, float(GC.SENTINEL), side="right")) - 1
    assert (counts[:, sentinel_bucket] == 0).all() and (values == GC.SENTINEL).sum() > 4 * len(offsets)
    assert np.array_equal(stats[:, [MIN, MAX, NUM]], ref_stats[:, [MIN, MAX, NUM]])
    assert (stats[:, NUM] == np.asarray(lengths)).all() and (stats[:, [NONFIN, BELOW, ABOVE]] == 0).all()
    for s, (o, n) in enumerate(zip(offsets, lengths)):
        v = values[o:o + n].astype(np.float64)
        err_sum, err_sq = abs(stats[s, SUM] - math.fsum(v)), abs(stats[s, SQ] - math.fsum(v * v))
        bound_sum, bound_sq = n * 2.0 ** -53 * np.abs(v).sum(), n * 2.0 ** -53 * (v * v).sum()
        print(f"segment {s}: len {n}  |sum - ref| {err_sum:.3e} <= {bound_sum:.3e}   |sq - ref| {err_sq:.3e} <= {bound_sq:.3e}")
        assert err_sum <= bound_sum and err_sq <= bound_sq, (s, n)


def test_contention():
    from mmvae_amd._hist_lib import HIST_ITEM_ELEMS as C
    from mmvae_amd.histogram import tensorboard_edges

    n = 3 * C + 7
    v = np.empty(3 * n, dtype=np.float32)
    v[:n] = 0.0
    v[n:2 * n] = 1.0
    v[2 * n:] = np.where(np.arange(n) % 2 == 0, np.float32(-0.37), np.float32(2.5e-3))
    offsets, lengths = [0, n, 2 * n], [n, n, n]
    counts, stats = _on_device(v, offsets, lengths)
    ref_counts, ref_stats = GC.reference(v, offsets, lengths, tensorboard_edges())
    assert np.array_equal(counts, ref_counts)
    assert (counts > 0).sum(1).tolist() == [1, 1, 2] and counts[0, 774] == n
    assert np.array_equal(stats[:, [MIN, MAX, NUM]], ref_stats[:, [MIN, MAX, NUM]])
    assert stats[1, SUM] == n and stats[1, SQ] == n and stats[0, SUM] == 0


@pytest.mark.parametrize("n_edges", [2, 2048])
def test_custom_edges(n_edges):
    edges = np.arange(n_edges, dtype=np.float64) - n_edges // 2
    rng = np.random.default_rng(n_edges)
    on_edges = rng.integers(int(edges[0]) - 3, int(edges[-1]) + 4, 5000).astype(np.float32)
    between = (rng.uniform(edges[0] - 2, edges[-1] + 2, 5000)).astype(np.float32)
    v = np.concatenate([on_edges, between, edges.astype(np.float32), [np.float32(edges[-1])] * 5]).astype(np.float32)
    offsets, lengths = [0, 3], [v.size, v.size - 3]
    counts, stats = _on_device(v, offsets, lengths, edges=edges)
    ref_counts, ref_stats = GC.reference(v, offsets, lengths, edges)
    assert np.array_equal(counts, ref_counts) and counts.shape == (2, n_edges - 1)
    assert np.array_equal(stats[:, [MIN, MAX, NUM, NONFIN, BELOW, ABOVE]], ref_stats[:, [MIN, MAX, NUM, NONFIN, BELOW, ABOVE]])
    assert counts[0, -1] >= 6  # (the values equal to the last edge are in the last bucket)
    # scale: an fp32 multiply (odd integers land between the edges, even ones on them)
    counts, stats = _on_device(v, offsets, lengths, edges=edges, scale=0.5)
    ref_counts, ref_stats = GC.reference(v, offsets, lengths, edges, scale=0.5)
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(stats[:, [MIN, MAX, NUM, BELOW, ABOVE]], ref_stats[:, [MIN, MAX, NUM, BELOW, ABOVE]])


def test_arguments_are_refused_before_any_launch():
    from mmvae_amd import _hist_lib
    from mmvae_amd.histogram import build_items, segment_histograms

    v = torch.zeros(100, device="cuda")
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [1.0, 0.0]):
        with pytest.raises(ValueError):
            segment_histograms(v, [0], [100], edges=bad)
    lib = _hist_lib.load_hist()
    items = torch.from_numpy(build_items([0], [100]).view(np.uint8).copy()).cuda()
    edges = torch.arange(2049, dtype=torch.float64, device="cuda")
    sentinel = 7
    counts = torch.full((2048,), sentinel, dtype=torch.int64, device="cuda")
    stats = torch.full((8,), float(sentinel), dtype=torch.float64, device="cuda")
    need = lib.mmvae_hist_workspace_bytes(1, 1, 2048)
    ws = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_edges, ws_bytes):
        return lib.mmvae_hist_segments_f32(1, items.data_ptr(), 1, v.data_ptr(), 1.0, n_edges, edges.data_ptr(),
                                           counts.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert call(1, need) == _hist_lib.ERR_ARG and call(2049, need) == _hist_lib.ERR_ARG
    assert call(2048, need - 1) == _hist_lib.ERR_ARG
    torch.cuda.synchronize()
    assert (counts == sentinel).all() and (stats == sentinel).all()  # nothing was launched, nothing cleared
    assert call(2048, need) == _hist_lib.OK
    torch.cuda.synchronize()
    assert counts[0] == 100 and counts[:2047].sum() == 100 and stats[NUM] == 100
    assert counts[2047] == sentinel  # (2 047 buckets: the word behind them is not the entry's)


def test_two_calls_are_bit_identical(geometry):
    values, offsets, lengths, _, (counts, stats) = geometry
    again_counts, again_stats = _on_device(values, offsets, lengths)
    assert np.array_equal(counts, again_counts)
    assert stats.tobytes() == again_stats.tobytes()


# ------------------------------------------------------------------------------------------- engine and model
GENES = {"human": 203, "mouse": 96}
ORDER = ("human", "mouse", "human", "mouse")


def _run(record: bool):
    """Four steps of the small two-expert model through the Trainer and the captured engine; with `record`, what
    save_gradients left at every recorded step next to the arenas' gradients and the logged norms of that step."""
    from mmvae_amd import rng, synthetic
    from mmvae_amd.trainer import Trainer

    model = synthetic.build_model(GENES, latent_dim=16, h1=64, h2=32, hv=24, dropout=0.1, seed=0).cuda()
    torch.manual_seed(1234)
    rng.reseed()
    model.record_gradients, model.save_gradients_interval, model.gradient_record_cap = record, 2, 10 ** 6
    xs = {eid: synthetic.synthetic_counts(32, g, seed=1 + i, device="cuda") for i, (eid, g) in enumerate(GENES.items())}
    batches = [(xs[eid], pd.DataFrame({"dummy": [0] * 32}), eid) for eid in ORDER]
    recorded = []
    inner = model.save_gradients

    def spy(optimizers=None, **kw):
        inner(optimizers, **kw)
        torch.cuda.synchronize()
        grads = [{n: o.arena.grad_view(i).detach().cpu().numpy().copy() for i, n in enumerate(_names(model, o))}
                 for o in optimizers]
        norms = {k: float(v) for k, v in model.logged.items() if k.startswith("grad_norms/")}
        recorded.append((model.gradient_histograms_step, dict(model.gradient_histograms), grads, norms))

    model.save_gradients = spy
    Trainer(max_epochs=1).fit(model, batches)
    torch.cuda.synchronize()
    assert model._engine, "the captured engine must have run the steps"
    return model, recorded


def _names(model, opt):
    name_of = {id(p): n for n, p in model.named_parameters()}
    return [name_of[id(p)] for p in opt.arena.params]


@pytest.fixture(scope="module")
def recording_run():
    return _run(True)


def _check_recorded(recorded):
    """Every recorded step: counts against np.histogram of the arena's gradient copied out behind that step, and
    sqrt(sum of sum_squares) per optimiser against the step's logged norm, 1e-4 relative (the bound
    tests/test_configs_gpu.py gives those norms against the oracle)."""
    from mmvae_amd.histogram import tensorboard_edges

    e = tensorboard_edges()
    assert [r[0] for r in recorded] == [0, 2]
    for step, found, grads, norms in recorded:
        eid = ORDER[step]
        assert set(found) == {f"gradients/{n}" for g in grads for n in g}
        assert all(t.startswith("gradients/module.vae.") or t.startswith(f"gradients/module.experts.{eid}.") for t in found)
        for g, logged in zip(grads, ("grad_norms/vae", f"grad_norms/expert_{eid}")):
            total = 0.0
            for name, grad in g.items():
                raw = found[f"gradients/{name}"]
                counts = np.histogram(grad.astype(np.float64).ravel(), bins=e)[0]
                filled = np.flatnonzero(counts)
                first, last = filled[0], filled[-1]
                assert raw["bucket_counts"][1:] == counts[first:last + 1].tolist(), (step, name)
                assert raw["bucket_limits"][-1] == e[last + 1] and raw["num"] == grad.size, (step, name)
                assert raw["min"] == grad.min() and raw["max"] == grad.max(), (step, name)
                total += raw["sum_squares"]
            got, want = math.sqrt(total), norms[logged]
            print(f"step {step} {logged}: sqrt(sum of sum_squares) {got:.8g}  logged {want:.8g}  rel {abs(got - want) / want:.2e}")
            assert abs(got - want) <= 1e-4 * want, (step, logged, got, want)


def test_engine_histograms_and_norms(recording_run):
    model, recorded = recording_run
    _check_recorded(recorded)
    assert model.gradient_histograms_step == 2


def test_engine_histograms_behind_a_deferred_expert_update(monkeypatch):
    """The overlapped program forced on one rank: the expert's norm, clip and Adam run on the communication stream behind
    the replay; the recording joins them and finds the same pre-clip gradients in the arenas."""
    monkeypatch.setenv("MMVAE_DP_OVERLAP", "1")
    model, recorded = _run(True)
    assert model._engine.overlap
    _check_recorded(recorded)


def test_recording_does_not_disturb_the_run(recording_run):
    model, _ = recording_run
    twin, recorded = _run(False)
    assert recorded == [] and twin.gradient_histograms == {}
    a, b = model.module.state_dict(), twin.module.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
