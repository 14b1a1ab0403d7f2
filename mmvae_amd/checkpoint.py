"""Checkpoints of a training run that do not stop the captured step.

`Checkpointer.save()` enqueues ONE launch of libmmvae_ckpt.so (include/mmvae_ckpt.h) on the training stream: it reads the
live optimiser arenas (parameters, Adam moments, state words), the module buffers and the Philox state in stream order
behind `engine.flush()`, writes a private device copy and computes per range a position-sensitive 64-bit checksum and a
count of non-finite values.  The training thread returns at once -- no device synchronisation, no `.item()` -- and a
worker thread drains the copy to pinned memory on a stream of its own, refuses to write when a fp32 range holds a
non-finite value (a diverged run never overwrites its last good file) and otherwise writes `path` atomically
(`path + ".tmp"`, fsync, os.replace).

There is ONE device buffer and ONE pinned buffer per Checkpointer, allocated once: a new `save()` first waits for the
previous one to finish, and raises what that one failed with.

The file is a `torch.save` dictionary in Lightning's shape -- `state_dict` (the keys, shapes and dtypes of
`model.state_dict()`), `optimizer_states` (equal to `[o.state_dict() for o in model.optimizers()]`), `epoch`,
`global_step`, `callbacks` -- plus `mmvae_amd`: format version, Philox {seed, offset}, annealing and learning-rate
schedule state, the optimisers' device state words, `MultiModalBatches.epoch` and the batches consumed in the current
epoch, `Trainer.history`, and the per-range digests with their names.  `load()` restores all of it in place (live
captured programs stay valid) and, with `verify`, recomputes the checksums over the loaded device state (the digest-only
mode of the kernel) and raises when one differs from the file's.

A model whose optimisers are not all HipAdam takes the blocking `state_dict()` path with the same file layout.  On CPU
plumbing (`backend.cpu_plumbing()`) the snapshot is the numpy mirror `snapshot_digest_reference`, taken on the calling
thread, so that the Trainer's logic runs without a GPU.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
import shutil
import threading
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import dist as mdist
from . import rng
from ._bind import stream

FORMAT_VERSION = 1
GOLDEN = 0x9E3779B97F4A7C15
_MASK64 = (1 << 64) - 1
_EXP = 0x7F800000


class CheckpointError(RuntimeError):
    pass


def snapshot_digest_reference(words, f32: bool) -> Tuple[int, int]:
    """The numpy mirror of the kernel's digest of one range: `words` is any array of 4-byte elements (taken as uint32
    words w_i).  Returns (sum_i (w_i + 1) * ((2 i + 1) * 0x9E3779B97F4A7C15) mod 2^64, the number of words whose fp32
    exponent field is all ones when `f32`, else 0).  uint64 array arithmetic wraps, which is the arithmetic wanted."""
    a = np.ascontiguousarray(words)
    if a.dtype.itemsize != 4:
        raise ValueError(f"snapshot_digest_reference: 4-byte elements wanted, got {a.dtype}")
    w = a.reshape(-1).view(np.uint32)
    total = np.uint64(0)
    nonfinite = 0
    golden = np.uint64(GOLDEN)
    with np.errstate(over="ignore"):
        for lo in range(0, w.size, 1 << 20):  # (pieces bound the temporaries)
            part = w[lo:lo + (1 << 20)]
            i = np.arange(lo, lo + part.size, dtype=np.uint64)
            terms = (part.astype(np.uint64) + np.uint64(1)) * ((np.uint64(2) * i + np.uint64(1)) * golden)
            total = total + terms.sum(dtype=np.uint64)
            if f32:
                nonfinite += int(np.count_nonzero((part & np.uint32(_EXP)) == np.uint32(_EXP)))
    return int(total) & _MASK64, nonfinite


class SaveHandle:
    """One `save()`: `wait()` blocks until the worker is done and raises what it failed with.  Afterwards `written` says
    whether the file was replaced, `nonfinite` maps the names of the fp32 ranges that held non-finite values to their
    counts (not written then), `digests` maps every range name to (checksum, non-finite count)."""

    def __init__(self, path: str):
        self.path = path
        self.written = False
        self.nonfinite: Dict[str, int] = {}
        self.digests: Dict[str, Tuple[int, int]] = {}
        self.error: Optional[BaseException] = None
        self._thread: Optional[threading.Thread] = None
        self._raised = False
        self.also: List[str] = []

    def done(self) -> bool:
        return self._thread is None or not self._thread.is_alive()

    def wait(self) -> "SaveHandle":
        if self._thread is not None:
            self._thread.join()
        if self.error is not None and not self._raised:
            self._raised = True
            raise self.error
        return self


class _Range:
    __slots__ = ("name", "tensor", "n_words", "f32", "dst_word")

    def __init__(self, name, tensor, f32):
        self.name, self.tensor, self.f32 = name, tensor, f32
        self.n_words = tensor.numel() * tensor.element_size() // 4
        self.dst_word = 0


def _is_hip_adam(opt) -> bool:
    from .optim import HipAdam

    return isinstance(opt, HipAdam)


class Checkpointer:
    """Built once after `model.optimizers()`, before training: the job table is built and uploaded here (never behind a
    captured program), the device copy, the pinned copy and the digest words are allocated here."""

    def __init__(self, model, digest_only: bool = False):
        """`digest_only`: for `digests()` alone -- no device copy and no pinned copy are allocated, `save()` refuses."""
        self.model = model
        self.digest_only = digest_only
        self.opts = list(model.optimizers())
        self._last: Optional[SaveHandle] = None
        self.fast = bool(self.opts) and all(_is_hip_adam(o) for o in self.opts)
        if self.fast:
            # The step engine moves every optimiser's state words into its metrics buffer when it is built (at the first
            # device step otherwise): built now, so that the table below names the words the captured programs write.
            first = self.opts[0].arena.data
            if first.is_cuda and getattr(model, "use_engine", False) and hasattr(model, "_get_engine"):
                model._get_engine(first)
            self._plan()
        if not self.fast:
            return
        self.device = self.ranges[0].tensor.device
        self.hip = self.device.type == "cuda"
        n = len(self.ranges)
        self.total_words = max(1, self._lay_out())
        words = 1 if digest_only else self.total_words
        if self.hip:
            from . import _ckpt_lib as L

            self._lib = L.load_ckpt()
            self._upload_table()
            self.copy_dev = torch.zeros(words, dtype=torch.int32, device=self.device)
            self.digest_dev = torch.zeros(2 * n, dtype=torch.int64, device=self.device)
            self.copy_host = torch.zeros(words, dtype=torch.int32).pin_memory()
            self.digest_host = torch.zeros(2 * n, dtype=torch.int64).pin_memory()
            self._copy_stream = torch.cuda.Stream(device=self.device)
        else:
            self.copy_host = torch.zeros(words, dtype=torch.int32)
            self.digest_host = torch.zeros(2 * n, dtype=torch.int64)

    # ------------------------------------------------------------------------------------------------ the job table
    def _plan(self) -> None:
        """The ranges (`self.ranges`) and where every entry of the two dictionaries lies in them: `self.state_index`
        maps a state_dict key to (range, first word, shape, dtype), `self.opt_index[o]` lists per parameter of optimiser
        o the (first word, shape) shared by its three arenas."""
        from .optim import arena_of

        model = self.model
        self.ranges: List[_Range] = []
        arena_range = {}
        self.opt_index = []
        for oi, opt in enumerate(self.opts):
            a = opt.arena
            first = len(self.ranges)
            for what, t in (("data", a.data), ("exp_avg", a.exp_avg), ("exp_avg_sq", a.exp_avg_sq),
                            ("state", opt.state_dev)):
                self.ranges.append(_Range(f"optimizer.{oi}.{what}", t, True))
            arena_range[id(opt)] = first
            self.opt_index.append([(off, tuple(p.shape)) for p, off in zip(a.params, a.offsets)])
        self.state_index = OrderedDict()
        for key, t in model.state_dict(keep_vars=True).items():
            hit = arena_of(t) if isinstance(t, torch.nn.Parameter) else None
            if hit is not None and id(hit[0]) in arena_range:
                opt, i = hit
                self.state_index[key] = (arena_range[id(opt)], opt.arena.offsets[i], tuple(t.shape), t.dtype)
                continue
            t = t.detach()
            if not t.is_contiguous() or (t.numel() * t.element_size()) % 4 or t.data_ptr() % 4 or \
                    t.device != self.opts[0].arena.device:
                self.fast = False  # (a buffer the word-wise snapshot cannot take: the blocking path)
                return
            self.state_index[key] = (len(self.ranges), 0, tuple(t.shape), t.dtype)
            self.ranges.append(_Range(f"state.{key}", t.reshape(-1), t.dtype == torch.float32))
        self.rng_range = len(self.ranges)
        self.ranges.append(_Range("rng", rng.state(self.opts[0].arena.device), False))

    def _upload_table(self) -> None:
        from . import _ckpt_lib as L

        n = len(self.ranges)
        table = np.zeros(n, dtype=np.dtype(L.JOB_DTYPE))
        for j, r in enumerate(self.ranges):
            table[j] = (r.tensor.data_ptr(), r.dst_word, r.n_words, L.CKPT_F32 if r.f32 else 0, 0)
        most = C.c_uint64(0)
        L.check(self._lib.mmvae_ckpt_check_jobs(n, table.ctypes.data, C.byref(most)), "mmvae_ckpt_check_jobs")
        self.max_words = int(most.value)
        self.jobs_dev = torch.from_numpy(table.view(np.uint8).copy()).to(self.device)

    def _check_live(self) -> None:
        """The optimisers' state words are the one range whose tensor another component may replace (a step engine built
        or rebuilt after this object): the table must name the live ones."""
        for oi, opt in enumerate(self.opts):
            r = self.ranges[4 * oi + 3]
            if r.tensor.data_ptr() != opt.state_dev.data_ptr():
                raise CheckpointError(f"optimiser {oi}'s state words have moved since this Checkpointer was built (a step "
                                      "engine was built or rebuilt): build a new Checkpointer")

    def _lay_out(self) -> int:
        """dst_word of every range: back to back, each placed so that its copy is congruent to its source mod 16 bytes
        (the kernel's 16-byte path).  Returns the words of the private copy."""
        cursor = 0
        for r in self.ranges:
            lane = (r.tensor.data_ptr() // 4) % 4
            cursor = (cursor + 3) // 4 * 4 + lane
            r.dst_word = cursor
            cursor += r.n_words
        return cursor

    # ------------------------------------------------------------------------------------------------------- saving
    def wait(self) -> Optional[SaveHandle]:
        """Wait for the save in flight, if any, and raise what it failed with."""
        last, self._last = self._last, None
        return last.wait() if last is not None else None

    def _host_bits(self) -> dict:
        model = self.model
        bits = {"steps": [None if getattr(o, "_steps", None) is None else np.array(o._steps, copy=True) for o in self.opts],
                "param_groups": [[{k: copy.deepcopy(v) for k, v in g.items() if k != "params"} for g in o.param_groups]
                                 for o in self.opts],
                "base_lrs": copy.deepcopy(getattr(model, "_base_lrs", None))}
        fn = getattr(model, "kl_annealing_fn", None)
        bits["annealing"] = {k: getattr(fn, k) for k in ("x", "_kl_weight") if hasattr(fn, k)}
        sched = getattr(model, "lr_schedule_fn", None)
        bits["lr_schedule"] = None if sched is None else {"step_count": int(sched.step_count)}
        # torch's host generator: what CPU plumbing draws its noise from (the device path draws from the Philox state)
        bits["torch_rng_state"] = torch.get_rng_state()
        return bits

    def launch(self, copy_out: bool = True) -> None:
        """The snapshot launch on the current stream (`copy_out=False`: digests only, nothing is written but them)."""
        from . import _ckpt_lib as L

        rc = self._lib.mmvae_ckpt_snapshot(len(self.ranges), self.jobs_dev.data_ptr(), self.max_words,
                                           self.copy_dev.data_ptr() if copy_out else None, self.digest_dev.data_ptr(),
                                           stream(self.device))
        L.check(rc, "mmvae_ckpt_snapshot")

    def _mirror(self, copy_out: bool = True) -> None:
        """CPU plumbing: the numpy mirror of the launch, on the calling thread."""
        host = self.copy_host.numpy()
        dig = self.digest_host.numpy().view(np.uint64)
        for j, r in enumerate(self.ranges):
            words = r.tensor.detach().reshape(-1).numpy().view(np.int32)
            if copy_out:
                host[r.dst_word:r.dst_word + r.n_words] = words
            dig[2 * j], dig[2 * j + 1] = (np.uint64(v) for v in snapshot_digest_reference(words, r.f32))

    def save(self, path: str, extra: Optional[dict] = None, also=()) -> SaveHandle:
        """Snapshot now, write later.  `also`: further paths that get a copy of the file (one snapshot, `best_model.ckpt`
        and `last.ckpt`), each replaced atomically like `path`.  `extra`: what the caller adds to the file -- `epoch`, `global_step`, `callbacks`
        at the top level, everything under its `mmvae_amd` key into the file's `mmvae_amd` section; copied here, on the
        calling thread.  Waits for the previous save first (one buffer pair) and raises what that one failed with."""
        if self.digest_only:
            raise CheckpointError("this Checkpointer was built for digests only")
        self.wait()
        model = self.model
        handle = SaveHandle(path)
        handle.also = [p for p in also if p != path]
        extra = copy.deepcopy(extra or {})
        model._flush_engine()
        if self.fast:
            model.gather_optimizer_state()  # (collective under data parallelism; the blocking state_dict()s gather too)
            self._check_live()
        if not self.fast:
            payload = self._blocking_payload(extra, handle)
            work = lambda: self._write(handle, payload)  # noqa: E731
        else:
            event = None
            if self.hip:
                self.launch()
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(self.device))
            else:
                self._mirror()
            bits = self._host_bits()
            work = lambda: self._drain_and_write(handle, event, bits, extra)  # noqa: E731

        def run():
            try:
                work()
            except BaseException as e:  # noqa: BLE001 -- raised at wait() and at the next save()
                handle.error = e

        handle._thread = threading.Thread(target=run, name="mmvae-checkpoint", daemon=True)
        handle._thread.start()
        self._last = handle
        return handle

    def _drain_and_write(self, handle: SaveHandle, event, bits: dict, extra: dict) -> None:
        if self.hip:
            torch.cuda.set_device(self.device)
            event.synchronize()
            with torch.cuda.stream(self._copy_stream):
                self.copy_host.copy_(self.copy_dev, non_blocking=True)
                self.digest_host.copy_(self.digest_dev, non_blocking=True)
            self._copy_stream.synchronize()
        dig = self.digest_host.numpy().view(np.uint64)
        handle.digests = {r.name: (int(dig[2 * j]), int(dig[2 * j + 1])) for j, r in enumerate(self.ranges)}
        handle.nonfinite = {r.name: handle.digests[r.name][1] for r in self.ranges if r.f32 and handle.digests[r.name][1]}
        if handle.nonfinite:
            return
        if mdist.rank() != 0:  # data parallelism: every rank snapshots behind the gather, rank 0 writes
            return
        self._write(handle, self._payload(bits, extra, handle.digests))

    # ---------------------------------------------------------------------------------------------- the dictionaries
    def _tensor(self, r: _Range, first: int, shape, dtype) -> torch.Tensor:
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size() // 4
        lo = r.dst_word + first
        words = self.copy_host.numpy()[lo:lo + n].copy()
        return torch.from_numpy(words).view(dtype).reshape(shape)

    def _payload(self, bits: dict, extra: dict, digests: dict) -> dict:
        R = self.ranges
        state = OrderedDict((key, self._tensor(R[ri], first, shape, dtype))
                            for key, (ri, first, shape, dtype) in self.state_index.items())
        optimizer_states, state_words = [], []
        for oi, opt in enumerate(self.opts):
            base = 4 * oi  # data, exp_avg, exp_avg_sq, state
            words = self._tensor(R[base + 3], 0, (R[base + 3].n_words,), torch.float32)
            state_words.append(words)
            steps = bits["steps"][oi]
            st = {}
            for i, (off, shape) in enumerate(self.opt_index[oi]):
                step = float(steps[i]) if steps is not None else float(words[0])
                st[i] = {"step": torch.tensor(step), "exp_avg": self._tensor(R[base + 1], off, shape, torch.float32),
                         "exp_avg_sq": self._tensor(R[base + 2], off, shape, torch.float32)}
            group = bits["param_groups"][oi][0]
            optimizer_states.append({"state": st, "param_groups": [{**group, "params": list(range(len(st)))}]})
        seed, offset = (int(v) for v in self._tensor(R[self.rng_range], 0, (2,), torch.int64))
        return self._assemble(state, optimizer_states, extra, bits, {"seed": seed, "offset": offset}, state_words,
                              [{"name": r.name, "checksum": digests[r.name][0], "nonfinite": digests[r.name][1],
                                "n_words": r.n_words, "f32": r.f32} for r in R])

    @staticmethod
    def _assemble(state, optimizer_states, extra, bits, philox, state_words, digests) -> dict:
        own = {"format_version": FORMAT_VERSION, "philox": philox, "annealing": bits["annealing"],
               "lr_schedule": bits["lr_schedule"], "base_lrs": bits["base_lrs"], "optimizer_state_words": state_words,
               "torch_rng_state": bits["torch_rng_state"],
               "batches_epoch": None, "batches_consumed": 0, "history": [], "digests": digests}
        own.update(extra.pop("mmvae_amd", {}))
        out = {"state_dict": state, "optimizer_states": optimizer_states, "epoch": 0, "global_step": 0, "callbacks": {},
               "mmvae_amd": own}
        out.update(extra)
        return out

    def _blocking_payload(self, extra: dict, handle: SaveHandle) -> dict:
        """The clone-based path: `state_dict()` of the model and of every optimiser, brought to the host here, on the
        calling thread (blocking).  Same file layout; no digests."""
        model = self.model
        state = OrderedDict((k, v.detach().cpu().clone()) for k, v in model.state_dict().items())
        optimizer_states = [_to_cpu(copy.deepcopy(o.state_dict())) for o in self.opts]
        bits = self._host_bits()
        device = next(iter(state.values())).device if state else torch.device("cpu")
        device = next((p.device for p in model.parameters()), device)
        st = rng.state(device).cpu()
        for k, v in state.items():
            if v.is_floating_point() and not bool(torch.isfinite(v).all()):
                handle.nonfinite[f"state.{k}"] = int((~torch.isfinite(v)).sum())
        words = [o.state_dev.detach().cpu().clone() for o in self.opts if hasattr(o, "state_dev")]
        return self._assemble(state, optimizer_states, extra, bits, {"seed": int(st[0]), "offset": int(st[1])}, words, [])

    def _write(self, handle: SaveHandle, payload: dict) -> None:
        if handle.nonfinite or mdist.rank() != 0:
            return
        path = handle.path
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + ".tmp"
        try:
            with open(tmp, "wb") as f:
                torch.save(payload, f)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
            for other in handle.also:
                os.makedirs(os.path.dirname(os.path.abspath(other)), exist_ok=True)
                tmp = other + ".tmp"
                with open(path, "rb") as src, open(tmp, "wb") as f:
                    shutil.copyfileobj(src, f, 1 << 24)
                    f.flush()
                    os.fsync(f.fileno())
                os.replace(tmp, other)
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise
        handle.written = True

    # ----------------------------------------------------------------------------------------------------- verifying
    def digests(self) -> Dict[str, Tuple[int, int]]:
        """(checksum, non-finite count) of every range as it is NOW: the digest-only mode of the kernel (nothing is
        copied), read back here -- this call synchronises."""
        if not self.fast:
            raise CheckpointError("digests exist on the snapshot path only (every optimiser a HipAdam)")
        self.wait()
        self.model._flush_engine()
        self._check_live()
        if self.hip:
            self.launch(copy_out=False)
            dig = self.digest_dev.cpu().numpy().view(np.uint64)
        else:
            self._mirror(copy_out=False)
            dig = self.digest_host.numpy().view(np.uint64)
        return {r.name: (int(dig[2 * j]), int(dig[2 * j + 1])) for j, r in enumerate(self.ranges)}


def _to_cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def load(path: str, model, trainer=None, verify: bool = True) -> dict:
    """Restore a checkpoint file in place: parameters and buffers through `load_state_dict` (copies into the arenas the
    captured programs point at), the optimisers' moments, step counts, hyper-parameters and device state words, the
    Philox state, the annealing and learning-rate schedule state; with `trainer`, its `global_step`, epoch, callback
    state, history and position in the data (`fit(ckpt_path=...)` continues from there).  `verify`: the checksums of the
    loaded device state are recomputed (digest-only launch) and compared with the file's; a difference raises
    CheckpointError.  Returns the file's dictionary."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    own = ckpt.get("mmvae_amd")
    if own is None or own.get("format_version") != FORMAT_VERSION:
        raise CheckpointError(f"{path}: not a checkpoint of this format (version {FORMAT_VERSION})")
    opts = list(model.optimizers())
    if len(opts) != len(ckpt["optimizer_states"]):
        raise CheckpointError(f"{path}: {len(ckpt['optimizer_states'])} optimiser states for {len(opts)} optimisers")
    model._flush_engine()
    model.load_state_dict(ckpt["state_dict"])
    for opt, sd in zip(opts, ckpt["optimizer_states"]):
        opt.load_state_dict(sd)
    for opt, words in zip([o for o in opts if hasattr(o, "state_dev")], own.get("optimizer_state_words") or []):
        opt.state_dev.copy_(words)
    device = next((p.device for p in model.parameters()), torch.device("cpu"))
    rng.state(device).copy_(torch.tensor([own["philox"]["seed"], own["philox"]["offset"]], dtype=torch.int64))
    fn = getattr(model, "kl_annealing_fn", None)
    for k, v in (own.get("annealing") or {}).items():
        setattr(fn, k, v)
    if own.get("lr_schedule") is not None and getattr(model, "lr_schedule_fn", None) is not None:
        model.lr_schedule_fn.step_count = int(own["lr_schedule"]["step_count"])
    if own.get("base_lrs") is not None:
        model._base_lrs = list(own["base_lrs"])
    if own.get("torch_rng_state") is not None:
        torch.set_rng_state(own["torch_rng_state"])
    if verify and own.get("digests"):
        found = Checkpointer(model, digest_only=True).digests()
        bad = [d["name"] for d in own["digests"] if found.get(d["name"], (None,))[0] != d["checksum"]]
        if bad:
            raise CheckpointError(f"{path}: the loaded state does not have the file's checksums: {bad}")
    if trainer is not None:
        trainer._resume_from(ckpt)
    return ckpt
