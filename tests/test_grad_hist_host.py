"""Host-side checks of the gradient histograms (no GPU): TensorBoard's default edges, the C-ABI surface of
libmmvae_hist.so, the numpy path of segment_histograms against np.histogram, tensorboard_raw against an independent
restatement (tests/grad_hist_cases.py), and the model's recording logic on a CPU model with a fake logger."""
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from tests import grad_hist_cases as GC
from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_hist.h")


def test_tensorboard_edges():
    from mmvae_amd.histogram import tensorboard_edges

    e = tensorboard_edges()
    assert e.dtype == np.float64 and e.shape == (1549,)
    assert (np.diff(e) > 0).all()
    assert (np.diff(e.astype(np.float32)) > 0).all()  # still strictly ascending after rounding to fp32
    assert e[0] == -9.920775621859783e+19 and e[-1] == 9.920775621859783e+19
    assert e[774] == 0.0 and e[775] == 1e-12 and e[773] == -1e-12
    assert np.array_equal(e[:774], -e[:774:-1])


def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _hist_lib

    declared = check_surface(_hist_lib.BINDING)
    assert set(declared) == {"mmvae_hist_abi_version", "mmvae_hist_build_arch", "mmvae_hist_workspace_bytes",
                             "mmvae_hist_segments_f32"} == set(_hist_lib.HIST_PROTOTYPES)


def test_versions_constants_and_argument_checks():
    from mmvae_amd import _hist_lib, _lib

    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _hist_lib.load_hist()
    assert define("MMVAE_HIST_ABI_VERSION") == 1 == lib.mmvae_hist_abi_version() == _hist_lib.HIST_ABI_VERSION
    assert lib.mmvae_hist_build_arch() == b"gfx950"
    assert define("MMVAE_HIST_ITEM_ELEMS") == _hist_lib.HIST_ITEM_ELEMS
    assert define("MMVAE_HIST_MAX_EDGES") == _hist_lib.HIST_MAX_EDGES == 2048
    assert define("MMVAE_HIST_STATS") == _hist_lib.HIST_STATS == len(_hist_lib.HIST_STAT_NAMES) == 8
    assert np.dtype(_hist_lib.HIST_ITEM_DTYPE).itemsize == 16
    # the training library is untouched: same version, none of the new names
    assert _lib.load().mmvae_abi_version() == 16
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_hist_")]
    need = lib.mmvae_hist_workspace_bytes
    assert need(10, 3, 1549) == 64 * 10 + 8 * 3 + 8 and need(10, 2, 2) == 64 * 10 + 16
    for bad in ((0, 1, 1549), (10, 0, 1549), (10, 3, 1), (10, 3, 2049), (2, 3, 1549)):
        assert need(*bad) == 0, bad
        assert lib.mmvae_hist_segments_f32(bad[0], 16, bad[1], 16, 1.0, bad[2], 16, 16, 16, 16, 1 << 30,
                                           None) == _hist_lib.ERR_ARG, bad
    ok = (10, 16, 3, 16, 1.0, 1549, 16, 16, 16, 16, need(10, 3, 1549), None)  # refused before any pointer is used:
    for i in (1, 3, 6, 7, 8, 9):  # a null pointer
        assert lib.mmvae_hist_segments_f32(*[None if j == i else a for j, a in enumerate(ok)]) == _hist_lib.ERR_ARG, i
    assert lib.mmvae_hist_segments_f32(*ok[:10], need(10, 3, 1549) - 1, None) == _hist_lib.ERR_ARG  # a short workspace
    assert lib.mmvae_hist_segments_f32(*ok[:9], 24, 1 << 30, None) == _hist_lib.ERR_ARG  # a misaligned one


def test_build_items_cuts_segments_in_order():
    from mmvae_amd._hist_lib import HIST_ITEM_ELEMS as C
    from mmvae_amd.histogram import build_items

    items = build_items([3, 100000, 7], [2 * C + 1, 1, C])
    assert items["segment"].tolist() == [0, 0, 0, 1, 2]
    assert items["offset"].tolist() == [3, 3 + C, 3 + 2 * C, 100000, 7]
    assert items["len"].tolist() == [C, C, 1, 1, C]
    for bad in (([], []), ([0], [0]), ([-1], [4]), ([0, 1], [4])):
        with pytest.raises(ValueError):
            build_items(*bad)


def test_cpu_path_equals_numpy_histogram():
    from mmvae_amd._hist_lib import HIST_ITEM_ELEMS as C
    from mmvae_amd.histogram import segment_histograms, tensorboard_edges

    e = tensorboard_edges()
    v = GC.edge_neighbour_values(e)
    h = segment_histograms(torch.from_numpy(v), [0], [v.size])
    counts, stats = GC.reference(v, [0], [v.size], e)
    assert np.array_equal(h.counts.numpy(), counts) and h.counts.dtype == torch.int64
    assert np.array_equal(h.stats.numpy()[:, [0, 1, 2, 5, 6, 7]], stats[:, [0, 1, 2, 5, 6, 7]])
    assert np.allclose(h.stats.numpy()[:, 3:5], stats[:, 3:5], rtol=1e-12)
    # where single values fall (np.histogram itself): 0, -0.0 and 1e-45 into bucket 774, -1e-45 into 773; NaN, +-inf and
    # 1e30 into none
    for val, bucket in ((0.0, 774), (-0.0, 774), (1e-45, 774), (-1e-45, 773), (np.nan, None), (np.inf, None),
                        (-np.inf, None), (1e30, None)):
        one = segment_histograms(torch.tensor([val], dtype=torch.float32), [0], [1]).counts[0].numpy()
        assert one.sum() == (bucket is not None) and (bucket is None or one[bucket] == 1), val
    assert int(h.n_nonfinite[0]) == 3 and int(h.n_above[0]) == 3 and int(h.n_below[0]) == 3
    # (above: FLT_MAX, 1e30 and the upper neighbour of the last edge's fp32 value, which itself lies under the edge)
    assert float(np.float32(e[-1])) < e[-1] < float(np.nextafter(np.float32(e[-1]), np.float32(np.inf)))
    # a value equal to the last edge falls into the last bucket; scale is an fp32 multiply
    ints = np.arange(-3, 4, dtype=np.float64)
    w = np.array([-4, -3, -2.5, 0, 2.999, 3, 3.5, 6], dtype=np.float32)
    h2 = segment_histograms(torch.from_numpy(w), [0, 2], [8, 6], edges=ints)
    assert h2.counts.tolist() == [[2, 0, 0, 1, 0, 2], [1, 0, 0, 1, 0, 2]]
    assert h2.n_below.tolist() == [1, 0] and h2.n_above.tolist() == [2, 2]
    h3 = segment_histograms(torch.from_numpy(w), [0], [8], edges=ints, scale=0.5)
    assert np.array_equal(h3.counts.numpy(), GC.reference(w, [0], [8], ints, scale=0.5)[0])
    # the geometry case of the GPU test
    vals, offsets, lengths = GC.geometry_case(C)
    hg = segment_histograms(torch.from_numpy(vals), offsets, lengths)
    counts, stats = GC.reference(vals, offsets, lengths, e)
    assert np.array_equal(hg.counts.numpy(), counts)
    assert np.array_equal(hg.stats.numpy()[:, :3], stats[:, :3])
    with pytest.raises(ValueError):
        segment_histograms(torch.from_numpy(w), [0], [8], edges=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        segment_histograms(torch.from_numpy(w), [0], [8], edges=[1.0])
    with pytest.raises(ValueError):
        segment_histograms(torch.from_numpy(w), [4], [5])


@pytest.mark.parametrize("support", ["middle", "from_first", "to_last", "single", "single_first", "empty"])
def test_tensorboard_raw_against_the_restatement(support):
    from mmvae_amd.histogram import SegmentHistograms

    edges = np.array([-2.0, -1.0, 0.0, 0.5, 1.0, 4.0, 9.0])
    counts = {"middle": [0, 3, 0, 2, 0, 0], "from_first": [5, 0, 1, 0, 0, 0], "to_last": [0, 0, 0, 1, 0, 7],
              "single": [0, 0, 0, 4, 0, 0], "single_first": [2, 0, 0, 0, 0, 0], "empty": [0, 0, 0, 0, 0, 0]}[support]
    stats = [-1.5, 8.0, float(sum(counts)), 3.25, 17.5, 2.0, 0.0, 1.0]
    packed = torch.zeros(2 * (6 + 8), dtype=torch.int64)
    h = SegmentHistograms(packed, 2, edges)
    h.counts[1] = torch.tensor(counts)
    h.stats[1] = torch.tensor(stats, dtype=torch.float64)
    want = GC.tensorboard_raw_restatement(counts, edges, stats)
    got = h.tensorboard_raw(1)
    assert h.tensorboard_raw(0) is None
    if support == "empty":
        assert want is None and got is None
        return
    assert got == want and set(got) == {"min", "max", "num", "sum", "sum_squares", "bucket_limits", "bucket_counts"}
    assert len(got["bucket_limits"]) == len(got["bucket_counts"]) and got["bucket_counts"][0] == 0
    assert sum(got["bucket_counts"]) == sum(counts) and got["num"] == sum(counts)
    if support == "middle":
        assert got["bucket_counts"] == [0, 3, 0, 2] and got["bucket_limits"] == [-1.0, 0.0, 0.5, 1.0]
    if support == "from_first":
        assert got["bucket_counts"] == [0, 5, 0, 1] and got["bucket_limits"] == [-2.0, -1.0, 0.0, 0.5]
    if support == "to_last":
        assert got["bucket_counts"] == [0, 1, 0, 7] and got["bucket_limits"] == [0.5, 1.0, 4.0, 9.0]


class _Experiment:
    def __init__(self):
        self.calls = []

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None):
        assert len(bucket_limits) == len(bucket_counts) and num == builtins_sum(bucket_counts)
        self.calls.append((tag, global_step))


builtins_sum = sum


class _Logger:
    def __init__(self):
        self.experiment = _Experiment()


def _cpu_run(**settings):
    """Four steps (human, mouse, human, mouse) of the small two-expert model on CPU plumbing through the Trainer."""
    from mmvae_amd import backend, synthetic
    from mmvae_amd.trainer import Trainer

    genes = {"human": 203, "mouse": 96}
    with backend.cpu_plumbing():
        model = synthetic.build_model(genes, latent_dim=16, h1=64, h2=32, hv=24, seed=0)
        for k, v in settings.items():
            setattr(model, k, v)
        model.logger = _Logger()
        xs = {eid: synthetic.synthetic_counts(8, g, seed=1 + i, device="cpu") for i, (eid, g) in enumerate(genes.items())}
        seen = []
        model_save = model.save_gradients

        def spy(*a, **kw):
            model_save(*a, **kw)
            seen.append((model.gradient_histograms_step, dict(model.gradient_histograms)))

        model.save_gradients = spy
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            Trainer(max_epochs=1).fit(model, [(xs[eid], pd.DataFrame({"dummy": [0] * 8}), eid)
                                              for eid in ("human", "mouse", "human", "mouse")])
        assert not [w for w in caught if "record_gradients" in str(w.message)]  # (none belongs to a single-process run)
    return model, seen


def test_model_records_at_the_interval_with_the_reference_tags():
    model, seen = _cpu_run(record_gradients=True, save_gradients_interval=2, gradient_record_cap=1000)
    assert [s for s, _ in seen] == [0, 2]
    calls = model.logger.experiment.calls
    assert sorted({s for _, s in calls}) == [0, 2]
    named = dict(model.named_parameters())
    want = {f"gradients/{n}" for n in named if n.startswith("module.vae.") or n.startswith("module.experts.human.")}
    assert want and not any("mouse" in t for t in want)  # steps 0 and 2 are human's
    for step, found in seen:
        assert set(found) == want
        assert {t for t, s in calls if s == step} == want
    assert model.gradient_histograms_step == 2 and set(model.gradient_histograms) == want
    assert model.record_gradients is True
    for tag, raw in model.gradient_histograms.items():
        assert raw["num"] == named[tag[len("gradients/"):]].numel() and raw["min"] <= raw["max"]


def test_model_cap_switches_recording_off():
    model, seen = _cpu_run(record_gradients=True, save_gradients_interval=2, gradient_record_cap=20)
    assert len(list(model.named_parameters())) > 20
    assert model.record_gradients is False
    assert model.gradient_histograms == {} and model.logger.experiment.calls == []
    assert len(seen) == 1  # the first due step found the cap exceeded; nothing was asked again


def test_model_without_record_gradients_does_nothing():
    model, seen = _cpu_run(save_gradients_interval=1, gradient_record_cap=1000)
    assert model.record_gradients is False and seen == []
    assert model.gradient_histograms == {} and model.gradient_histograms_step is None
    assert model.logger.experiment.calls == []
