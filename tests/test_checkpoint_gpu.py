"""The checkpoint snapshot on the GPU: libmmvae_ckpt.so's launch against its numpy mirror (copy, both digest words, sources
untouched, nothing written outside the ranges), a snapshot's isolation from the training that goes on behind it, and the
exact resume of a Trainer run from `last.ckpt` -- at an epoch boundary and mid-epoch."""
import copy
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, 3 * 2 ** 20 + 5)
SENTINEL = 0x5A5A5A5A
_cache: dict = {}


def _source_words():
    """3 * 2^20 + 5 + 3 random words on the host, with inf / NaN / denormal / -0 patterns sown in, and their device copy
    (16-byte aligned: torch's allocator hands out 512-byte multiples).  Built once; never written afterwards."""
    if "host" not in _cache:
        rng = np.random.default_rng(20)
        w = rng.integers(0, 2 ** 32, size=SIZES[-1] + 3, dtype=np.uint64).astype(np.uint32)
        special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x00000001, 0x80000000, 0],
                           dtype=np.uint32)
        w[rng.integers(0, w.size, size=4096)] = special[rng.integers(0, special.size, size=4096)]
        w[:8] = special
        _cache["host"] = w
        _cache["dev"] = torch.from_numpy(w.view(np.int32)).cuda()
        assert _cache["dev"].data_ptr() % 16 == 0
    return _cache["host"], _cache["dev"]


def _reference(offset, n, f32):
    """The mirror's digest of words [offset, offset + n) of the source: computed once per range."""
    from mmvae_amd.checkpoint import snapshot_digest_reference

    key = (offset, n, f32)
    if key not in _cache:
        _cache[key] = snapshot_digest_reference(_source_words()[0][offset:offset + n], f32)
    return _cache[key]


def _launch(jobs, dst_words, copy_out=True):
    """jobs: (source offset, n_words, dst_word, f32) over the shared source.  Returns (dst as uint32 on the host or None,
    digests [n_jobs, 2] uint64) of ONE launch; dst is pre-filled with a sentinel."""
    from mmvae_amd import _ckpt_lib as L

    lib = L.load_ckpt()
    host, dev = _source_words()
    table = np.zeros(len(jobs), dtype=np.dtype(L.JOB_DTYPE))
    for j, (off, n, dst_word, f32) in enumerate(jobs):
        table[j] = (dev.data_ptr() + 4 * off, dst_word, n, L.CKPT_F32 if f32 else 0, 0)
    most = C.c_uint64(0)
    assert lib.mmvae_ckpt_check_jobs(len(jobs), table.ctypes.data, C.byref(most)) == L.OK
    assert most.value == max([n for _, n, _, _ in jobs], default=0)
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    dst = torch.full((dst_words,), SENTINEL, dtype=torch.int32, device="cuda") if copy_out else None
    digest = torch.full((max(1, 2 * len(jobs)),), -1, dtype=torch.int64, device="cuda")  # (the call clears it itself)
    rc = lib.mmvae_ckpt_snapshot(len(jobs), table_dev.data_ptr(), most.value, dst.data_ptr() if copy_out else None,
                                 digest.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == L.OK
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), host), "the launch wrote to its source"
    out = dst.cpu().numpy().view(np.uint32) if copy_out else None
    return out, digest.cpu().numpy().view(np.uint64)[:2 * len(jobs)].reshape(-1, 2)


def _check(jobs, out, digests):
    host = _source_words()[0]
    if out is not None:
        untouched = np.ones(out.size, dtype=bool)
    for j, (off, n, dst_word, f32) in enumerate(jobs):
        want = _reference(off, n, f32)
        assert (int(digests[j, 0]), int(digests[j, 1])) == want, (j, off, n, dst_word, f32)
        if out is not None:
            assert np.array_equal(out[dst_word:dst_word + n], host[off:off + n]), (j, off, n, dst_word)
            untouched[dst_word:dst_word + n] = False
    if out is not None:
        assert (out[untouched] == SENTINEL).all(), "a word outside every range was written"


@pytest.mark.parametrize("dst_off", range(4))
@pytest.mark.parametrize("src_off", range(4))
def test_kernel_equals_the_mirror_at_every_alignment(src_off, dst_off):
    """All word counts in one launch, every source 16-byte alignment against every destination alignment: equal residues
    take the 16-byte path with a peeled head and tail, unequal ones the single-word path."""
    jobs, cursor = [], 0
    for k, n in enumerate(SIZES):
        cursor = (cursor + 3) // 4 * 4 + dst_off + 4  # (a gap of sentinel words in front of every range)
        jobs.append((src_off, n, cursor, k % 2 == 0))
        cursor += n
    out, digests = _launch(jobs, cursor + 8)
    _check(jobs, out, digests)
    assert digests[0].tolist() == [0, 0]  # an empty range
    assert any(d[1] > 0 for d in digests.tolist()), "the sown non-finite patterns must be counted somewhere"
    assert all(d[1] == 0 for d in digests[1::2].tolist()), "raw jobs count nothing"


def test_three_hundred_mixed_jobs_in_one_launch():
    rng = np.random.default_rng(4)
    jobs, cursor = [], 0
    for k in range(300):
        n = int(rng.choice([0, 1, 2, 7, 64, 255, 1000, 4099, 8192, 8193, 20001]))
        off = int(rng.integers(0, 64))
        cursor += int(rng.integers(0, 6))
        jobs.append((off, n, cursor, bool(rng.integers(0, 2))))
        cursor += n
    jobs[137] = (3, 3 * 2 ** 20 - 11, cursor + 1, True)  # one long range among the short ones
    cursor += 1 + jobs[137][1]
    out, digests = _launch(jobs, cursor + 4)
    _check(jobs, out, digests)


def test_digest_only_mode_and_repeated_calls():
    jobs = [(o, n, 0, True) for o in range(4) for n in (0, 5, 1025, 70001)] + [(1, SIZES[-1], 0, False)]
    _, first = _launch(jobs, 0, copy_out=False)
    _check(jobs, None, first)
    _, again = _launch(jobs, 0, copy_out=False)
    assert np.array_equal(first, again)
    _, copied = _launch([(o, n, 8 + 80000 * j, f) for j, (o, n, _, f) in enumerate(jobs[:-1])], 8 + 80000 * len(jobs))
    assert np.array_equal(first[:-1], copied), "copying or not, the digests are the same"


# ------------------------------------------------------------------------------------------------------- the Trainer
GENES = {"human": 203, "mouse": 96}  # 203: not a multiple of 4
B = 16


def _seed(seed=7):
    from mmvae_amd import rng

    torch.manual_seed(seed)
    rng.state(torch.device("cuda", torch.cuda.current_device()))  # (made now, so that the line below seeds it)
    rng.reseed(seed)  # (build_model re-seeds torch: the device state gets its seed here, explicitly)


def _model(seed=0):
    from mmvae_amd import synthetic
    from mmvae_amd.modules.base.annealing_fn import LinearKLAnnealingFn
    from mmvae_amd.modules.base.lr_schedule import WarmupCosineLRFn

    model = synthetic.build_model(GENES, latent_dim=8, h1=48, h2=32, hv=24, dropout=0.1, seed=seed).cuda()
    model.kl_annealing_fn = LinearKLAnnealingFn(min_kl_weight=1e-3, max_kl_weight=0.5, warmup_steps=2, climax_steps=9)
    model.lr_schedule_fn = WarmupCosineLRFn(warmup_steps=3, total_steps=40, min_factor=0.1)
    return model


def _batches(split_seed, n=4):
    from mmvae_amd import synthetic
    from mmvae_amd.trainer import MultiModalBatches

    loaders = {eid: [(synthetic.synthetic_counts(B, g, seed=split_seed + 10 * k + i, device="cuda"),
                      pd.DataFrame({"dummy": [0] * B}), eid) for k in range(n)]
               for i, (eid, g) in enumerate(GENES.items())}
    return MultiModalBatches(loaders, seed=split_seed)


def _fit(model, dirpath, max_epochs=2, ckpt_path=None, **kw):
    from mmvae_amd.callbacks import ModelCheckpoint
    from mmvae_amd.trainer import Trainer

    ckpt_kw = {k: kw.pop(k) for k in ("every_n_train_steps", "every_n_epochs") if k in kw}
    trainer = Trainer(max_epochs=max_epochs, callbacks=[ModelCheckpoint(dirpath=str(dirpath), save_last=True, save_top_k=0,
                                                                        **ckpt_kw)], **kw)
    trainer.fit(model, _batches(100), _batches(500, n=1), ckpt_path=ckpt_path)
    return trainer


def _final_state(model):
    from mmvae_amd import rng

    model._flush_engine()
    torch.cuda.synchronize()
    state = {f"sd/{k}": v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for oi, opt in enumerate(model.optimizers()):
        sd = opt.state_dict()
        for i, st in sd["state"].items():
            for k, v in st.items():
                state[f"opt{oi}/{i}/{k}"] = v.detach().cpu().clone()
        state[f"opt{oi}/lr"] = torch.tensor(sd["param_groups"][0]["lr"], dtype=torch.float64)
    state["philox"] = rng.state(next(model.parameters()).device).cpu().clone()
    state["kl_weight"] = torch.tensor(model.kl_annealing_fn.kl_weight, dtype=torch.float64)
    state["kl_x"] = torch.tensor(model.kl_annealing_fn.x, dtype=torch.float64)
    state["lr_step_count"] = torch.tensor(model.lr_schedule_fn.step_count)
    return state


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """Two epochs without interruption (8 steps each, a validation behind each): the state every resumed run must reach."""
    _seed()
    model = _model()
    trainer = _fit(model, tmp_path_factory.mktemp("straight"), every_n_train_steps=3)
    assert model._engine, "the captured engine must have run the steps"
    assert trainer.global_step == 16 and trainer.stop_reason is None
    state = _final_state(model)
    assert int(state["philox"][1]) > 0, "the device Philox noise must have been drawn"
    return state, [dict(h) for h in trainer.history]


def _assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f"{k} differs from the uninterrupted run"


@pytest.mark.parametrize("where", ["epoch_end", "mid_epoch"])
def test_resumed_run_is_bit_identical(straight, tmp_path, where):
    """One epoch (or three steps of it), `last.ckpt`, a FRESH model with other initial weights, `fit(ckpt_path=...)` to
    the end of the second epoch: parameters, buffers, Adam moments and steps, the Philox offset, the KL weight and the
    learning rate are those of the uninterrupted run, bit for bit; so is the history."""
    want, history = straight
    _seed()
    first = _model()
    if where == "epoch_end":
        t1 = _fit(first, tmp_path, max_epochs=1)
        assert t1.global_step == 8
    else:
        t1 = _fit(first, tmp_path, max_steps=3, every_n_train_steps=3, every_n_epochs=0)
        assert t1.global_step == 3
    path = os.path.join(str(tmp_path), "last.ckpt")
    ckpt = torch.load(path, weights_only=False)
    assert ckpt["global_step"] == t1.global_step
    assert ckpt["mmvae_amd"]["batches_consumed"] == (0 if where == "epoch_end" else 3)
    assert ckpt["mmvae_amd"]["next_epoch"] == (1 if where == "epoch_end" else 0)
    del first

    _seed(1234)  # (another random state: the file's must win)
    resumed = _model(seed=99)
    t2 = _fit(resumed, tmp_path / "resumed", ckpt_path=path, every_n_train_steps=3)
    assert t2.global_step == 16
    _assert_same(_final_state(resumed), want)
    assert [h.get("stage") for h in t2.history] == [h.get("stage") for h in history]
    # (an epoch's training entry also carries whatever earlier stages left in `model.logged`; a fresh model has none of
    # the first epoch's validation values there, so the resumed entries are compared on the keys they hold)
    for got, ref in zip(t2.history[-2:], history[-2:]):
        assert any(k.startswith("loss/") for k in got)
        assert all(ref[k] == v for k, v in got.items()), (got, ref)
    assert t2.history[-1] == history[-1]


def test_a_snapshot_is_isolated_from_what_follows_it(tmp_path):
    """save(), then 1 added to every arena before wait(): the file holds the state at the call."""
    from mmvae_amd.checkpoint import Checkpointer

    _seed()
    model = _model()
    _fit(model, tmp_path / "warm", max_epochs=1)
    want_sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want_opt = [copy.deepcopy(o.state_dict()) for o in model.optimizers()]
    ck = Checkpointer(model)
    assert ck.fast and ck.hip
    path = str(tmp_path / "iso.ckpt")
    handle = ck.save(path, {"epoch": 0, "global_step": 8})
    for opt in model.optimizers():
        for t in (opt.arena.data, opt.arena.exp_avg, opt.arena.exp_avg_sq):
            t.add_(1.0)
    handle.wait()
    assert handle.written and not handle.nonfinite
    ckpt = torch.load(path, weights_only=False)
    assert list(ckpt["state_dict"]) == list(want_sd) and ckpt["global_step"] == 8
    for k, v in want_sd.items():
        got = ckpt["state_dict"][k]
        assert got.dtype == v.dtype and got.shape == v.shape and torch.equal(got, v), k
    assert not torch.equal(next(iter(model.state_dict().values())).cpu(), next(iter(want_sd.values())))
    for got, want in zip(ckpt["optimizer_states"], want_opt):
        assert got["param_groups"] == want["param_groups"] and list(got["state"]) == list(want["state"])
        for i, st in want["state"].items():
            for k, v in st.items():
                g = got["state"][i][k]
                assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v.cpu()), (i, k)
    assert {d["name"] for d in ckpt["mmvae_amd"]["digests"]} == set(handle.digests)


def test_load_verifies_the_checksums(tmp_path):
    from mmvae_amd.checkpoint import CheckpointError, load

    _seed()
    model = _model()
    _fit(model, tmp_path, max_epochs=1)
    path = os.path.join(str(tmp_path), "last.ckpt")
    other = _model(seed=5)
    load(path, other, verify=True)
    for (k, a), b in zip(model.state_dict().items(), other.state_dict().values()):
        assert torch.equal(a, b), k
    ckpt = torch.load(path, weights_only=False)
    key = [k for k, v in ckpt["state_dict"].items() if v.is_floating_point() and v.numel() > 4][3]
    ckpt["state_dict"][key].view(-1)[2] += 1.0
    bad = str(tmp_path / "altered.ckpt")
    torch.save(ckpt, bad)
    with pytest.raises(CheckpointError, match="checksums"):
        load(bad, _model(seed=6), verify=True)
    load(bad, _model(seed=6), verify=False)  # (asked not to look, it loads)
