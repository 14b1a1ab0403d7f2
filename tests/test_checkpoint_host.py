"""Host-side checks of the checkpoint feature (no GPU): the C-ABI surface of libmmvae_ckpt.so and its refusals, the numpy
mirror of the digest against a big-integer loop, and the Trainer's callback / checkpoint / resume logic on CPU plumbing
with a tiny model."""
import ctypes as C
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests.abi_surface import check_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmvae_ckpt.h")
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------ ABI and surface
def test_header_symbols_are_exported_and_bound():
    from mmvae_amd import _bind, _ckpt_lib

    declared = check_surface(_ckpt_lib.BINDING)
    assert set(declared) == {"mmvae_ckpt_abi_version", "mmvae_ckpt_build_arch", "mmvae_ckpt_check_jobs",
                             "mmvae_ckpt_snapshot"} == set(_ckpt_lib.CKPT_PROTOTYPES)
    assert "_ckpt_lib" in _bind.DEVICE_LIBRARY_MODULES
    header = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))  # noqa: E731
    lib = _ckpt_lib.load_ckpt()
    assert define("MMVAE_CKPT_ABI_VERSION") == 1 == lib.mmvae_ckpt_abi_version() == _ckpt_lib.CKPT_ABI_VERSION
    assert define("MMVAE_CKPT_F32") == _ckpt_lib.CKPT_F32 and define("MMVAE_CKPT_CHUNK_WORDS") == _ckpt_lib.CKPT_CHUNK_WORDS
    assert define("MMVAE_CKPT_MAX_GROUPS") == _ckpt_lib.CKPT_MAX_GROUPS
    assert C.sizeof(_ckpt_lib.CkptJob) == 32 == np.dtype(_ckpt_lib.JOB_DTYPE).itemsize
    # the training library is untouched: none of the new names
    from mmvae_amd import _lib

    assert not [n for n in _lib.PROTOTYPES if n.startswith("mmvae_ckpt_")]


def _table(*jobs):
    from mmvae_amd import _ckpt_lib as L

    t = np.zeros(len(jobs), dtype=np.dtype(L.JOB_DTYPE))
    for j, job in enumerate(jobs):
        t[j] = job
    return t


def test_every_argument_error_is_refused():
    from mmvae_amd import _ckpt_lib as L

    lib = L.load_ckpt()
    most = C.c_uint64(77)
    good = _table((4096, 0, 10, L.CKPT_F32, 0), (8192 + 4, 16, 0, 0, 0), (0, 0, 0, 0, 0))
    assert lib.mmvae_ckpt_check_jobs(3, good.ctypes.data, C.byref(most)) == L.OK and most.value == 10
    assert lib.mmvae_ckpt_check_jobs(0, None, C.byref(most)) == L.OK and most.value == 0
    assert lib.mmvae_ckpt_check_jobs(3, good.ctypes.data, None) == L.OK
    for bad in ((4097, 0, 10, 0, 0), (4098, 0, 10, 0, 0), (4099, 0, 10, 0, 0),  # a misaligned src
                (4096, 0, 1 << 32, 0, 0), (4096, 0, (1 << 32) + 5, 0, 0),        # n_words >= 2^32
                (0, 0, 3, 0, 0),                                                  # no source for words to read
                (4096, 0, 10, 2, 0), (4096, 0, 10, 0, 1)):                        # an unknown flag, a used reserved word
        t = _table((4096, 0, 1, 0, 0), bad)
        assert lib.mmvae_ckpt_check_jobs(2, t.ctypes.data, C.byref(most)) == L.ERR_ARG, bad
    longest = _table((4096, 0, (1 << 32) - 1, 0, 0))
    assert lib.mmvae_ckpt_check_jobs(1, longest.ctypes.data, C.byref(most)) == L.OK and most.value == (1 << 32) - 1
    assert lib.mmvae_ckpt_check_jobs(-1, good.ctypes.data, None) == L.ERR_ARG
    assert lib.mmvae_ckpt_check_jobs(2, None, None) == L.ERR_ARG
    # the launch entry: refused on the host before anything is touched (the pointers below are never followed)
    snap = lib.mmvae_ckpt_snapshot
    assert snap(-1, 4096, 10, 4096, 4096, None) == L.ERR_ARG          # n_jobs < 0
    assert snap(2, None, 10, 4096, 4096, None) == L.ERR_ARG           # a NULL table with jobs
    assert snap(2, 4096, 1 << 32, 4096, 4096, None) == L.ERR_ARG      # max_words >= 2^32
    assert snap(2, 4096, 10, 4096, None, None) == L.ERR_ARG           # nowhere to put the digests
    assert snap(2, 4096, 10, 4096, 4100, None) == L.ERR_ARG           # misaligned digests
    assert snap(2, 4096, 10, 4098, 4096, None) == L.ERR_ARG           # misaligned dst
    assert snap(0, None, 0, None, None, None) == L.OK                 # nothing to do is valid


# ------------------------------------------------------------------------------------------------------- digest mirror
def _big_integer_digest(words, f32):
    total = nonfinite = 0
    for i, w in enumerate(int(v) for v in words):
        total = (total + (w + 1) * (((2 * i + 1) * GOLDEN) & M64)) & M64
        nonfinite += int(f32 and (w & 0x7F800000) == 0x7F800000)
    return total, nonfinite


def test_mirror_equals_a_big_integer_loop():
    from mmvae_amd.checkpoint import snapshot_digest_reference as ref

    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 5, 64, 1000):
        w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        if n:
            w[0] = 0xFFFFFFFF  # (w + 1 = 2^32 must not wrap to 0)
        for f32 in (False, True):
            assert ref(w, f32) == _big_integer_digest(w, f32), (n, f32)
        assert ref(w.view(np.float32), True) == ref(w.view(np.int32), True) == ref(w, True)
    assert ref(np.zeros(0, np.uint32), True) == (0, 0)
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.float64), True)
    # across the mirror's internal piece boundary (2^20 words): the word index keeps counting
    w = rng.integers(0, 1 << 32, size=(1 << 20) + 3, dtype=np.uint64).astype(np.uint32)
    tail = _big_integer_digest(w[-3:], False)[0]
    head = ref(w[:1 << 20], False)[0]
    shifted = sum((int(v) + 1) * (((2 * ((1 << 20) + k) + 1) * GOLDEN) & M64) for k, v in enumerate(w[-3:])) & M64
    assert ref(w, False)[0] == (head + shifted) & M64 and shifted != tail


def test_checksum_is_position_and_length_sensitive():
    from mmvae_amd.checkpoint import snapshot_digest_reference as ref

    w = np.arange(10, 30, dtype=np.uint32)
    swapped = w.copy()
    swapped[[3, 11]] = swapped[[11, 3]]
    assert ref(w, False)[0] != ref(swapped, False)[0]
    same = w.copy()
    same[5] = same[6] = 99
    again = same.copy()
    again[[5, 6]] = again[[6, 5]]
    assert ref(same, False) == ref(again, False)  # (equal words swapped: the same range)
    zeros = {ref(np.zeros(n, np.uint32), False)[0] for n in (0, 1, 2, 3, 7, 8, 1024, 1025)}
    assert len(zeros) == 8
    assert ref(np.zeros(3, np.uint32), False)[0] == (9 * GOLDEN) & M64  # sum of (2 i + 1) over 3 words = 3^2


def test_nonfinite_count():
    from mmvae_amd.checkpoint import snapshot_digest_reference as ref

    words = np.array([0x7F800000, 0xFF800000,              # +inf, -inf
                      0x7FC00000, 0xFFC00001, 0x7FFFFFFF,  # quiet NaNs
                      0x7F800001, 0xFFA00000,              # signalling NaNs
                      0x00000001, 0x807FFFFF,              # denormals
                      0x80000000, 0x00000000,              # -0, +0
                      0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000], dtype=np.uint32)  # +-FLT_MAX, 1.0
    assert ref(words, True)[1] == 7 and ref(words, False)[1] == 0
    assert ref(words, True)[0] == ref(words, False)[0]
    assert (~np.isfinite(words.view(np.float32))).sum() == 7


# ------------------------------------------------------------------------------------------------------- Trainer logic
GENES = {"human": 37, "mouse": 21}


def _model(seed=0):
    from mmvae_amd import synthetic

    return synthetic.build_model(GENES, latent_dim=4, h1=16, h2=8, hv=8, seed=seed)


def _loaders(seed=1, n=2):
    from mmvae_amd import synthetic
    from mmvae_amd.trainer import MultiModalBatches

    return MultiModalBatches({eid: [(synthetic.synthetic_counts(8, g, seed=seed + 10 * k + i), pd.DataFrame({"dummy": [0] * 8}),
                                     eid) for k in range(n)] for i, (eid, g) in enumerate(GENES.items())}, seed=seed)


class _Scripted:
    """A Trainer whose validation reports a scripted monitor sequence (the loop, the callbacks and the files are real)."""

    def __init__(self, values, **kw):
        from mmvae_amd.trainer import Trainer

        outer = self
        self.values = list(values)

        class T(Trainer):
            def validate(self, model, batches):
                super().validate(model, batches)
                self.callback_metrics["monitored"] = outer.values[self.current_epoch]

        self.trainer = T(max_epochs=len(self.values), **kw)

    def fit(self, model=None):
        from mmvae_amd import backend

        with backend.cpu_plumbing():
            model = model or _model()
            self.trainer.fit(model, _loaders(1), _loaders(5, n=1))
        return self.trainer


def _saved_epochs(dirpath):
    out = {}
    for name in ("best_model", "last"):
        path = os.path.join(dirpath, name + ".ckpt")
        out[name] = torch.load(path, weights_only=False)["epoch"] if os.path.exists(path) else None
    return out


@pytest.mark.parametrize("values, kw, best, last, stop", [
    # patience: two checks without improvement end the run; the best file stays at the best epoch
    ([5.0, 4.0, 4.5, 4.2, 1.0, 1.0], dict(patience=2), 1, 3, 3),
    # min_delta: an improvement of less than min_delta does not reset the patience (the file still follows the minimum)
    ([5.0, 4.95, 4.9, 1.0], dict(patience=2, min_delta=0.2), 2, 2, 2),
    ([5.0, 4.5, 4.0, 3.5], dict(patience=2, min_delta=0.2), 3, 3, None),
    # mode: max
    ([1.0, 2.0, 1.5, 1.7, 9.0], dict(patience=2, mode="max"), 1, 3, 3),
    # stopping_threshold: better than the threshold ends the run at once
    ([5.0, 4.0, 0.5, 0.1], dict(patience=10, stopping_threshold=1.0), 2, 2, 2),
    # divergence_threshold
    ([5.0, 4.0, 50.0, 0.1], dict(patience=10, divergence_threshold=20.0), 1, 2, 2),
    # check_finite
    ([5.0, float("nan"), 1.0], dict(patience=10), 0, 1, 1),
])
def test_monitor_sequence_gives_the_right_files_and_stop_epoch(tmp_path, values, kw, best, last, stop):
    from mmvae_amd.callbacks import EarlyStopping, ModelCheckpoint

    mode = kw.get("mode", "min")
    run = _Scripted(values, callbacks=[ModelCheckpoint(dirpath=str(tmp_path), filename="best_model", monitor="monitored",
                                                       mode=mode, save_last=True),
                                       EarlyStopping(monitor="monitored", **kw)])
    trainer = run.fit()
    saved = _saved_epochs(str(tmp_path))
    assert saved == {"best_model": best, "last": last}
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    if stop is None:
        assert trainer.stop_reason is None and trainer.current_epoch == len(values) - 1
    else:
        assert trainer.stop_reason and trainer.current_epoch == stop
        assert trainer.early_stopping_callbacks[0].stopped_epoch == stop
    assert trainer.global_step == 4 * (trainer.current_epoch + 1)
    assert trainer.checkpoint_callback.best_model_score == (max if mode == "max" else min)(
        v for v in values[:trainer.current_epoch + 1] if not math.isnan(v))


def test_no_callbacks_is_the_loop_as_it_was(tmp_path):
    from mmvae_amd import backend
    from mmvae_amd.callbacks import ModelCheckpoint
    from mmvae_amd.trainer import Trainer

    def run(**kw):
        torch.manual_seed(3)
        with backend.cpu_plumbing():
            model = _model()
            t = Trainer(max_epochs=2, **kw)
            t.fit(model, _loaders(1), _loaders(5, n=1))
        return t, {k: v.clone() for k, v in model.state_dict().items()}

    plain, sd_plain = run()
    assert plain.callback_metrics == {} and plain.checkpointer is None and plain.stop_reason is None
    assert not os.listdir(tmp_path)
    with_cb, sd_cb = run(callbacks=[ModelCheckpoint(dirpath=str(tmp_path), save_last=True, save_top_k=0)])
    assert plain.history == with_cb.history and plain.global_step == with_cb.global_step == 8
    assert all(torch.equal(sd_plain[k], sd_cb[k]) for k in sd_plain)
    assert os.listdir(tmp_path) == ["last.ckpt"]
    with pytest.raises(ValueError):
        ModelCheckpoint(save_top_k=2)
    with pytest.raises(ValueError):
        ModelCheckpoint(save_top_k=-1)
    with pytest.raises(ValueError):
        Trainer(callbacks=[ModelCheckpoint()], enable_checkpointing=False)


def test_validation_metrics_are_row_weighted_epoch_means(tmp_path):
    """Three validation batches of 8, 3 and 5 rows whose steps log 1, 2 and 4: the monitored value is (8 + 6 + 20) / 16,
    not the last value and not the plain mean; `history` keeps the last logged value, as before."""
    from mmvae_amd import backend
    from mmvae_amd.callbacks import ModelCheckpoint
    from mmvae_amd.trainer import Trainer

    with backend.cpu_plumbing():
        model = _model()
        scripted = iter([1.0, 2.0, 4.0, 3.0])

        def validation_step(batch, batch_idx=0):
            v = next(scripted)
            model.log_dict({f"loss/validation/{batch[2]}": torch.tensor(v), f"kl_weight/validation/{batch[2]}": 0.5})
            model.log("val_loss", torch.tensor(2 * v))

        model.validation_step = validation_step
        val = [(torch.zeros(rows, 37), pd.DataFrame({"dummy": [0] * rows}), "human") for rows in (8, 3, 5)]
        val.append((torch.zeros(4, 21), pd.DataFrame({"dummy": [0] * 4}), "mouse"))
        t = Trainer(max_epochs=1, callbacks=[ModelCheckpoint(dirpath=str(tmp_path), monitor="loss/validation/human")])
        t.fit(model, _loaders(1), val)
    assert t.callback_metrics["loss/validation/human"] == 2.125
    assert t.callback_metrics["loss/validation/mouse"] == 3.0
    assert t.callback_metrics["kl_weight/validation/human"] == 0.5
    assert t.callback_metrics["val_loss"] == 2 * (8 + 6 + 20 + 12) / 20
    assert t.history[-1]["stage"] == "validation" and t.history[-1]["loss/validation/human"] == 4.0
    assert t.checkpoint_callback.best_model_score == 2.125


def test_from_yaml_builds_both_callbacks():
    from mmvae_amd.callbacks import EarlyStopping, ModelCheckpoint
    from mmvae_amd.trainer import Trainer

    t = Trainer.from_yaml(os.path.join(ROOT, "configs", "trainer", "checkpointing.yaml"))
    kinds = [type(c) for c in t.callbacks]
    assert kinds == [ModelCheckpoint, EarlyStopping]
    ck, es = t.callbacks
    assert (ck.filename, ck.monitor, ck.save_top_k, ck.save_last, ck.mode) == (
        "best_model", "loss/validation/human", 1, True, "min")
    assert ck.every_n_train_steps == 0 and ck.every_n_epochs == 1 and ck.save_on_train_epoch_end is False
    assert (es.monitor, es.min_delta, es.patience, es.mode, es.strict, es.check_finite) == (
        "loss/validation/human", 0.001, 2, "min", True, True)
    assert es.stopping_threshold is None and es.divergence_threshold is None
    assert t.checkpoint_callback is ck and t.max_epochs == 10
    plain = Trainer.from_yaml(os.path.join(ROOT, "configs", "trainer", "config.yaml"))
    assert plain.callbacks == [] and plain.max_epochs == 2


def test_file_equals_the_blocking_dictionaries_and_resumes(tmp_path):
    """`state_dict` and `optimizer_states` of a file: the keys, shapes, dtypes and values of the blocking dictionaries;
    then load() into another model, and fit(ckpt_path=...) to the uninterrupted run's state."""
    from mmvae_amd import backend, checkpoint as CK
    from mmvae_amd.callbacks import ModelCheckpoint
    from mmvae_amd.modules.base.annealing_fn import LinearKLAnnealingFn
    from mmvae_amd.modules.base.lr_schedule import WarmupCosineLRFn
    from mmvae_amd.trainer import Trainer

    def model_(seed=0):
        m = _model(seed)
        m.kl_annealing_fn = LinearKLAnnealingFn(1e-3, 0.5, warmup_steps=1, climax_steps=5)
        m.lr_schedule_fn = WarmupCosineLRFn(2, 20, 0.1)
        return m

    def fit(model, d, max_epochs, ckpt_path=None, **kw):
        t = Trainer(max_epochs=max_epochs, callbacks=[ModelCheckpoint(dirpath=str(d), save_last=True, save_top_k=0, **kw)])
        t.fit(model, _loaders(1), _loaders(5, n=1), ckpt_path=ckpt_path)
        return t

    with backend.cpu_plumbing():
        torch.manual_seed(0)
        straight = model_()
        fit(straight, tmp_path / "s", 2)
        want = {k: v.clone() for k, v in straight.state_dict().items()}
        want_opt = [o.state_dict() for o in straight.optimizers()]
        ckpt = torch.load(tmp_path / "s" / "last.ckpt", weights_only=False)
        assert list(ckpt["state_dict"]) == list(want)
        for k, v in want.items():
            g = ckpt["state_dict"][k]
            assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v), k
        assert any(v.dtype == torch.int64 for v in want.values())  # (BatchNorm's num_batches_tracked travels raw)
        assert len(ckpt["optimizer_states"]) == len(want_opt) == 3
        for got, blocking in zip(ckpt["optimizer_states"], want_opt):
            assert got["param_groups"] == blocking["param_groups"] and list(got["state"]) == list(blocking["state"])
            for i, st in blocking["state"].items():
                assert set(got["state"][i]) == set(st)
                for k, v in st.items():
                    g = got["state"][i][k]
                    assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v), (i, k)
        own = ckpt["mmvae_amd"]
        assert ckpt["epoch"] == 1 and ckpt["global_step"] == 8 and set(ckpt["callbacks"]) == {"ModelCheckpoint"}
        assert own["format_version"] == 1 and own["next_epoch"] == 2 and own["batches_consumed"] == 0
        assert own["annealing"]["x"] == straight.kl_annealing_fn.x and own["lr_schedule"] == {"step_count": 8}
        assert [h["stage"] for h in own["history"]] == ["training", "validation"] * 2
        names = [d["name"] for d in own["digests"]]
        assert names[:4] == ["optimizer.0.data", "optimizer.0.exp_avg", "optimizer.0.exp_avg_sq", "optimizer.0.state"]
        assert names[-1] == "rng" and any(n.endswith("running_var") for n in names)

        for kw, at in ((dict(), 4), (dict(every_n_train_steps=3, every_n_epochs=0), 3)):
            torch.manual_seed(0)
            first = model_()
            d = tmp_path / f"r{at}"
            Trainer(max_epochs=1, max_steps=at, callbacks=[ModelCheckpoint(dirpath=str(d), save_last=True, save_top_k=0,
                                                                         **kw)]).fit(first, _loaders(1), _loaders(5, n=1))
            mid = torch.load(d / "last.ckpt", weights_only=False)
            assert mid["global_step"] == at and mid["mmvae_amd"]["batches_consumed"] == (0 if at == 4 else 3)
            resumed = model_(seed=9)
            t = fit(resumed, d / "more", 2, ckpt_path=str(d / "last.ckpt"))
            assert t.global_step == 8
            for k, v in want.items():
                assert torch.equal(resumed.state_dict()[k], v), (at, k)
            for o, blocking in zip(resumed.optimizers(), want_opt):
                sd = o.state_dict()
                for i, st in blocking["state"].items():
                    assert all(torch.equal(sd["state"][i][k], v) for k, v in st.items()), (at, i)
            assert resumed.kl_annealing_fn.kl_weight == straight.kl_annealing_fn.kl_weight
            assert resumed.lr_schedule_fn.step_count == 8

        # verify: an altered tensor is found
        key = [k for k, v in ckpt["state_dict"].items() if v.is_floating_point() and v.numel() > 4][2]
        ckpt["state_dict"][key].view(-1)[1] += 0.5
        torch.save(ckpt, tmp_path / "altered.ckpt")
        with pytest.raises(CK.CheckpointError, match="checksums"):
            CK.load(str(tmp_path / "altered.ckpt"), model_(seed=4))


def test_a_model_with_other_optimisers_takes_the_blocking_path(tmp_path):
    from mmvae_amd import backend, checkpoint as CK

    with backend.cpu_plumbing():
        model = _model()
        model.configure_optimizers = lambda: [torch.optim.Adam(model.parameters(), lr=1e-3)]
        ck = CK.Checkpointer(model)
        assert not ck.fast
        handle = ck.save(str(tmp_path / "b.ckpt"), {"epoch": 3, "global_step": 30}).wait()
        assert handle.written
        got = torch.load(tmp_path / "b.ckpt", weights_only=False)
        assert list(got["state_dict"]) == list(model.state_dict()) and got["epoch"] == 3
        assert set(got) == {"state_dict", "optimizer_states", "epoch", "global_step", "callbacks", "mmvae_amd"}
        assert got["mmvae_amd"]["digests"] == [] and len(got["optimizer_states"]) == 1


# ---------------------------------------------------------------------------------------------------- failure handling
def test_a_failed_write_keeps_the_previous_file_and_surfaces_at_wait(tmp_path, monkeypatch):
    from mmvae_amd import backend, checkpoint as CK

    with backend.cpu_plumbing():
        model = _model()
        model.optimizers()
        ck = CK.Checkpointer(model)
        path = str(tmp_path / "last.ckpt")
        ck.save(path, {"epoch": 0, "global_step": 1}).wait()
        before = open(path, "rb").read()

        def broken(*a, **kw):
            raise OSError("disk full")

        monkeypatch.setattr(CK.torch, "save", broken)
        handle = ck.save(path, {"epoch": 1, "global_step": 2})
        with pytest.raises(OSError, match="disk full"):
            handle.wait()
        assert not handle.written and open(path, "rb").read() == before
        assert os.listdir(tmp_path) == ["last.ckpt"]  # (no .tmp left behind)
        # an error nobody waited for surfaces at the next save()
        ck.save(path, {"epoch": 2, "global_step": 3})
        with pytest.raises(OSError, match="disk full"):
            ck.save(path, {"epoch": 3, "global_step": 4})
        monkeypatch.undo()
        assert ck.save(path, {"epoch": 4, "global_step": 5}).wait().written
        assert torch.load(path, weights_only=False)["epoch"] == 4


def test_a_nan_in_a_parameter_keeps_last_ckpt_and_stops_the_run(tmp_path):
    """The run trains and validates the human expert only; after the second epoch's validation a NaN lands in a parameter
    of the mouse expert (no step touches it, so training itself goes on undisturbed).  The snapshot behind it must refuse
    to write -- both files stay those of the first epoch -- and the run must end in the third epoch, not the fifth."""
    from mmvae_amd import backend, synthetic
    from mmvae_amd.callbacks import ModelCheckpoint
    from mmvae_amd.trainer import Trainer

    class Poisoned(Trainer):
        def validate(self, model, batches):
            super().validate(model, batches)
            if self.current_epoch == 1:
                next(model.module.experts["mouse"].parameters()).data.view(-1)[0] = float("nan")

    with backend.cpu_plumbing():
        model = _model()
        human = [(synthetic.synthetic_counts(8, 37, seed=60 + k), pd.DataFrame({"dummy": [0] * 8}), "human") for k in range(3)]
        t = Poisoned(max_epochs=5, callbacks=[ModelCheckpoint(dirpath=str(tmp_path), monitor="loss/validation/human",
                                                              mode="max", save_last=True)])
        t.fit(model, human, human[:1])
        mouse = model.optimizers().index(model.get_optimizers()["experts"]["mouse"])
    assert t.stop_reason and "non-finite" in t.stop_reason and f"optimizer.{mouse}.data" in t.stop_reason
    assert t.current_epoch == 2, "the run must end when the refusal is known, not train on"
    saved = _saved_epochs(str(tmp_path))
    assert saved["last"] == 0, "last.ckpt must stay the last good one"
    assert saved["best_model"] == 0
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    assert math.isfinite(t.history[-1].get("loss/training/human", 0.0))
