"""Data feed of the training step: chunked npz-CSR counts + pickled metadata -> `(x, metadata, expert_id)`
batches, the tuples `CMMVAEModel.training_step` consumes.

Mirrors the reference's local datapipes without torchdata (not installed here; data/local/cellxgene_datapipe.py):
  * chunk discovery  -- `FileLister(root, masks, non_deterministic=False)` zipped pairwise (:295-318): files of one
    directory matched by fnmatch masks, sorted, counts chunk i paired with metadata chunk i;
  * chunk loading    -- `scipy.sparse.load_npz` + `pickle.load` of a DataFrame (:60-86);
  * shuffling        -- chunk order and, per chunk, one row permutation applied to matrix and DataFrame alike (:110-122);
  * batching         -- consecutive `batch_size` rows as `torch.sparse_csr_tensor(indptr, indices, data)` (int32 indices by default,
    fp32 values) or, with `return_dense`, its dense form; partial batches dropped unless `allow_partials` (:169-193);
  * tagging          -- `(tensor, metadata, species_name)` (data/local/cellxgene_manager.py:76-88).
Differences, all on purpose: the shuffles draw from a seeded `numpy.random.Generator` (the reference uses the global
numpy state) so that an epoch is reproducible and data-parallel ranks can be given disjoint, rank-synchronous
streams; the next chunk is loaded and permuted by a background thread while the current one is consumed; batches can be
staged to the device as CSR components from pinned memory (12 B per stored element instead of 4 B per gene), where
`mmvae_csr_to_dense_f32` densifies them straight into the step's input buffer.

Device-resident chunks (`SpeciesChunks(device_chunks=True)`, opt-in): instead of gathering every batch on the host and
copying it over, the background chunk thread uploads each chunk ONCE -- its CSR arrays, its row order and the row-pointer
table of every batch it will yield (`batch_row_pointers`), validated on the host first (`validate_csr_chunk`) -- and a
batch is one launch of `mmvae_csr_gather_rows_*` (or `mmvae_csr_gather_rows_dense_*` with `return_dense`) that copies
the chosen rows out of the resident chunk.  Per batch the host is left with that launch and the metadata slice.  The
batches are the same, bit for bit, as those of the host path; at most two chunks are resident (the one being consumed
and the next), and a chunk over `device_chunk_bytes` takes the host path for that chunk alone.
"""
from __future__ import annotations

import fnmatch
import atexit
import ctypes as C
import os
import pickle
import queue
import threading
import warnings
from typing import Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd
import torch

from ._bind import CSRC, Binding


def _wrap(v) -> List[str]:
    return [v] if isinstance(v, str) else list(v)


def list_chunks(directory_path: str, npz_masks: Union[str, Sequence[str]],
                metadata_masks: Union[str, Sequence[str]]) -> List[Tuple[str, str]]:
    """Sorted (counts.npz, metadata.pkl) pairs of one directory (non-recursive), zipped pairwise like the reference's
    two FileListers; raises when nothing matches (cellxgene_datapipe.py:312-318)."""
    names = sorted(os.listdir(directory_path))

    def pick(masks):
        return [os.path.join(os.path.abspath(directory_path), n) for n in names
                if os.path.isfile(os.path.join(directory_path, n)) and any(fnmatch.fnmatch(n, m) for m in _wrap(masks))]

    pairs = list(zip(pick(npz_masks), pick(metadata_masks)))
    if not pairs:
        raise RuntimeError("No files found for masks from file lister")
    return pairs


def _mapped_npz_csr(npz_path: str):
    """Memory-mapped CSR matrix of an UNCOMPRESSED scipy npz (`save_npz(..., compressed=False)`): the .npy members of
    a stored zip are plain byte ranges of the file, so indptr / indices / data become page-cache-backed views instead
    of being read and copied through zipfile (0.29 s -> ~1 ms per 2048-cell chunk).  Returns None when the archive is
    compressed or is not a CSR matrix: the caller falls back to scipy.sparse.load_npz."""
    import struct
    import zipfile

    import scipy.sparse as sp

    arrays = {}
    with zipfile.ZipFile(npz_path) as zf, open(npz_path, "rb") as f:
        for info in zf.infolist():
            if info.compress_type != zipfile.ZIP_STORED:
                return None
            f.seek(info.header_offset)
            hdr = f.read(30)
            n_name, n_extra = struct.unpack("<HH", hdr[26:30])
            start = info.header_offset + 30 + n_name + n_extra
            f.seek(start)
            version = np.lib.format.read_magic(f)
            shape, fortran, dtype = (np.lib.format.read_array_header_1_0(f) if version == (1, 0)
                                     else np.lib.format.read_array_header_2_0(f))
            name = info.filename[:-4] if info.filename.endswith(".npy") else info.filename
            if dtype.hasobject or fortran:
                return None
            if int(np.prod(shape)) * dtype.itemsize <= 4096:  # format / shape scalars: just read them
                arrays[name] = np.fromfile(f, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
            else:
                arrays[name] = np.memmap(npz_path, dtype=dtype, mode="r", offset=f.tell(), shape=shape)
    fmt = arrays.get("format")
    fmt = fmt.item() if fmt is not None else b""
    if (fmt.decode() if isinstance(fmt, bytes) else str(fmt)) != "csr":
        return None
    return sp.csr_matrix((arrays["data"], arrays["indices"], arrays["indptr"]), shape=tuple(arrays["shape"]), copy=False)


def load_chunk(npz_path: str, metadata_path: str):
    """One chunk: scipy CSR matrix + its index-matched metadata DataFrame (cellxgene_datapipe.py:60-86)."""
    import scipy.sparse as sp

    matrix = _mapped_npz_csr(npz_path)
    if matrix is None:
        with open(npz_path, "rb") as f:
            matrix = sp.load_npz(f).tocsr()
    with open(metadata_path, "rb") as f:
        metadata = pickle.load(f)
    if matrix.shape[0] != len(metadata):
        raise ValueError(f"{npz_path}: {matrix.shape[0]} rows but {len(metadata)} metadata rows in {metadata_path}")
    return matrix, metadata


_GATHER = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p])
# name -> (restype, argtypes), in the order of include/mmvae_feed.h
FEED_PROTOTYPES = {
    "mmvae_feed_abi_version": (C.c_int, []),
    "mmvae_feed_rows_nnz": (C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    "mmvae_feed_gather_rows": _GATHER,
    "mmvae_feed_gather_rows_i32": _GATHER,
    "mmvae_feed_cond_tables": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]),
}
FEED_ABI_VERSION = 3
FEED_BINDING = Binding("libmmvae_feed.so", "mmvae_feed.h", FEED_PROTOTYPES, "mmvae_feed_abi_version", FEED_ABI_VERSION,
                       needs_torch=False)  # host code: no build arch, and no HIP runtime to share with torch
_FEED = None


def feed_lib():
    """libmmvae_feed.so (include/mmvae_feed.h): the native row gather.  Built by `make -C mmvae_amd/csrc` together with
    the HIP library; built on demand here (g++, one file) when it is missing -- it is host code, not the HIP path."""
    global _FEED
    if _FEED is None:
        if not os.path.exists(FEED_BINDING.path):
            import subprocess

            subprocess.run(["make", "-C", CSRC, "libmmvae_feed.so"], check=True, capture_output=True)
        _FEED = FEED_BINDING.load()
    return _FEED


def validate_csr_chunk(indptr: np.ndarray, indices: np.ndarray, data: np.ndarray, n_cols: int, where: str) -> None:
    """The host-side check of a chunk that is about to become device-resident: raises ValueError (naming `where`, the
    chunk's file) unless the row pointers start at 0, never decrease and end at the number of stored elements, and every
    column index lies in [0, n_cols).  The gather kernels clamp what they read anyway; this is what makes a malformed
    file an error instead of silently shortened rows."""
    if indptr.ndim != 1 or len(indptr) < 1 or int(indptr[0]) != 0:
        raise ValueError(f"{where}: malformed CSR chunk: indptr[0] != 0")
    if len(indptr) > 1 and bool((indptr[1:] < indptr[:-1]).any()):
        raise ValueError(f"{where}: malformed CSR chunk: indptr decreases")
    if not (int(indptr[-1]) == len(indices) == len(data)):
        raise ValueError(f"{where}: malformed CSR chunk: indptr[-1] = {int(indptr[-1])} but {len(indices)} indices and "
                         f"{len(data)} values")
    if len(indices) and (int(indices.min()) < 0 or int(indices.max()) >= n_cols):
        raise ValueError(f"{where}: malformed CSR chunk: column index outside [0, {n_cols})")


def batch_row_pointers(indptr: np.ndarray, order: np.ndarray, batch_size: int, allow_partials: bool = False,
                       dtype=np.int32) -> Tuple[np.ndarray, List[int], List[int]]:
    """Row pointers of EVERY batch a chunk yields, in one vectorised pass: batch k is rows order[k B : (k + 1) B] of the
    chunk, and its `crow_indices` are the running sum of those rows' lengths.  Returns (table, nnz, n_rows): `table`
    is [n_batches, B + 1] of `dtype`, nnz[k] / n_rows[k] are Python ints.  A partial last batch -- kept only with
    `allow_partials` -- has n_rows < B: its row pointers are table[k, :n_rows + 1] (the padding repeats its nnz)."""
    B = int(batch_size)
    n = len(order)
    n_batches = -(-n // B) if allow_partials else n // B
    lengths = np.zeros(n_batches * B, dtype=np.int64)
    kept = min(n, n_batches * B)
    row_len = np.diff(np.asarray(indptr).astype(np.int64, copy=False))
    lengths[:kept] = row_len[np.asarray(order[:kept], dtype=np.int64)]
    table = np.zeros((n_batches, B + 1), dtype=np.int64)
    np.cumsum(lengths.reshape(n_batches, B), axis=1, out=table[:, 1:])
    nnz = [int(v) for v in table[:, B]]
    n_rows = [min(B, n - k * B) for k in range(n_batches)]
    if n_batches and nnz and max(nnz) > np.iinfo(dtype).max:
        raise ValueError(f"a batch of {max(nnz)} stored elements needs index_dtype=torch.int64")
    return table.astype(dtype, copy=False), nnz, n_rows


class _DeviceChunk:
    """One chunk resident on the device: a `torch.sparse_csr` view of it, its row order (int64) and the row-pointer table
    of its batches, all parts of ONE buffer uploaded by one copy on the feed's copy stream; `event` is recorded behind
    that copy.  The metadata frame and the host copy of the row order stay on the host (the metadata slice)."""
    __slots__ = ("buf", "csr", "rows", "table", "nnz", "n_rows", "event", "metadata", "order", "ready")

    def __init__(self, buf, csr, rows, table, nnz, n_rows, event, metadata, order):
        self.buf, self.csr, self.rows, self.table, self.nnz, self.n_rows = buf, csr, rows, table, nnz, n_rows
        self.event, self.metadata, self.order = event, metadata, order
        self.ready = None  # handle of the producing stream once it waits for `event` (first batch of the chunk)


class _Slot:
    """Staging arrays of one batch in flight: row pointers / column indices (int32 or int64) and fp32 values in the layout
    torch.sparse_csr uses.  Page-locked when the batches go to a GPU; reused once the asynchronous H2D copies that
    read it have completed (`event`)."""

    def __init__(self, n_rows: int, pinned: bool, index_dtype=torch.int32):
        self.pinned = pinned
        self.index_dtype = index_dtype
        self.n_rows = n_rows
        # page-locked int32 batches live in ONE buffer -- row pointers | column indices | values, each part starting on a
        # 16-byte boundary -- and go to the device with ONE copy (three `.to()` calls were 0.15 ms of the producer's share
        # of an interpreter-bound loop: profiles/HISTORY.md r5)
        self.packed = pinned and index_dtype == torch.int32
        self.buf = None
        self.crow = self._alloc(n_rows + 1, index_dtype) if not self.packed else None
        self.col = self._alloc(16, index_dtype) if not self.packed else None
        self.val = self._alloc(16, torch.float32) if not self.packed else None
        self.event = None
        if self.packed:
            self.reserve(16)

    def _alloc(self, n: int, dtype) -> torch.Tensor:
        t = torch.empty(n, dtype=dtype)
        return t.pin_memory() if self.pinned else t

    @staticmethod
    def _pad4(n: int) -> int:
        return (n + 3) // 4 * 4

    def layout(self, nnz: int):
        """(offset of the column indices, offset of the values, words in use) inside the packed buffer."""
        o_col = self._pad4(self.n_rows + 1)
        o_val = o_col + self._pad4(nnz)
        return o_col, o_val, o_val + nnz

    def reserve(self, nnz: int) -> None:
        if self.packed:
            o_col, o_val, words = self.layout(nnz)
            if self.buf is None or self.buf.numel() < words:
                cap = int(nnz * 1.25) + 16  # reused: leave headroom
                self.buf = self._alloc(self.layout(cap)[2], torch.int32)
            self.crow = self.buf[:self.n_rows + 1]
            self.col = self.buf[o_col:o_col + nnz]
            self.val = self.buf[o_val:o_val + nnz].view(torch.float32)
            return
        if self.col.numel() < nnz:
            cap = (int(nnz * 1.25) + 16) if self.pinned else max(nnz, 1)  # pinned buffers are reused: leave headroom
            self.col, self.val = self._alloc(cap, self.index_dtype), self._alloc(cap, torch.float32)


class _Workers:
    """A few persistent threads behind a C-level queue: `submit(fn, *args)` returns an object whose `result()` waits for
    and returns fn's value (or re-raises its exception).  What the feed needs of ThreadPoolExecutor at a fifth of its cost
    per job (the executor's submit was 0.1 ms per batch on the GPU box, under the interpreter lock the training thread also
    needs)."""

    class _Job:
        __slots__ = ("done", "value", "error")

        def __init__(self):
            self.done, self.value, self.error = threading.Event(), None, None

        def result(self):
            self.done.wait()
            if self.error is not None:
                raise self.error
            return self.value

    def __init__(self, n: int):
        self.jobs: "queue.SimpleQueue" = queue.SimpleQueue()
        self.threads = [threading.Thread(target=self._work, daemon=True) for _ in range(max(1, n))]
        for t in self.threads:
            t.start()

    def _work(self):
        while True:
            item = self.jobs.get()
            if item is None:
                return
            job, fn, args = item
            try:
                job.value = fn(*args)
            except BaseException as e:  # noqa: BLE001 -- re-raised by result()
                job.error = e
            job.done.set()

    def submit(self, fn, *args):
        job = self._Job()
        self.jobs.put((job, fn, args))
        return job

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for _ in self.threads:
            self.jobs.put(None)
        for t in self.threads:
            t.join(timeout=10.0)
        return False


class SpeciesChunks:
    """Iterable over the batches of one modality's chunk files: `(x, metadata, name)`.

    A batch is gathered row by row out of the (memory-mapped) chunk by the native helper -- the row permutation is an
    index list, the chunk itself is never permuted or sliced in Python -- into a ring of staging slots, `workers`
    batches ahead of the consumer and off the interpreter lock.

    `rank` / `world`: data-parallel sharding -- every rank walks the same (seeded) chunk order and row permutations;
    the epoch's kept batches (across chunks, dropped partial batches not counted) are dealt out in rounds of `world`,
    rank r takes the r-th batch of every COMPLETE round and the incomplete last round is dropped, so every rank yields
    exactly floor(n_batches / world) batches of the same modality schedule -- a rank that ran short would leave the
    others blocked in the gradient all-reduce (the reference has no distributed sampler).

    `device_chunks=True` (needs a GPU `device`): chunks are uploaded once and batches gathered on the device by one HIP
    launch each (`_iter_device`); same batches.  `device_chunk_bytes`: budget of one resident chunk (default: a quarter
    of the free device memory when the iterator starts); at most two chunks are resident, a chunk over the budget is
    gathered on the host (one warning per object).

    `normalize="log1p_cpm"` (default None: the files hold what the model trains on already): the chunk files hold RAW
    counts and every batch is normalised on its way out, v <- log1p(target_sum * v / rowsum) per cell
    (mmvae_amd.preprocess: the reference's normalize_data).  A device-resident chunk is normalised once, where it lies, by
    one launch behind its upload; a host-gathered batch by the same kernel over its CSR values on the producing stream
    (numpy on a CPU `device`).  A row's result depends on that row's values in their stored order alone, so both paths
    yield the same batches bit for bit.  Files that do not look like raw counts draw one RuntimeWarning per object."""

    def __init__(self, directory_path: str, npz_masks, metadata_masks, batch_size: int, name: str,
                 allow_partials: bool = False, shuffle: bool = True, return_dense: bool = False, seed: int = 0,
                 device: Optional[Union[str, torch.device]] = None, prefetch: bool = True, rank: int = 0, world: int = 1,
                 workers: int = 3, gather_threads: int = 2, index_dtype: torch.dtype = torch.int32,
                 device_chunks: bool = False, device_chunk_bytes: Optional[int] = None, normalize: Optional[str] = None,
                 target_sum: float = 1e4):
        self.chunks = list_chunks(directory_path, npz_masks, metadata_masks)
        self.batch_size = int(batch_size)
        self.name = name
        self.allow_partials = allow_partials
        self.shuffle = shuffle
        self.return_dense = return_dense
        self.seed = seed
        self.device = torch.device(device) if device is not None else None
        self.prefetch = prefetch
        self.rank, self.world = rank, world
        self.workers = max(1, int(workers))
        self.gather_threads = max(1, int(gather_threads))
        # int32: what the reference's batches carry (torch.sparse_csr_tensor keeps the int32 indptr / indices of the scipy
        # slice, cellxgene_datapipe.py:178-183) and a third less data per batch on the wire; int64 on request
        if index_dtype not in (torch.int32, torch.int64):
            raise ValueError("index_dtype must be torch.int32 or torch.int64")
        self.index_dtype = index_dtype
        self.epoch = 0
        self._slots: List[_Slot] = []
        # device-resident chunks (opt-in): see _iter_device
        self.device_chunks = bool(device_chunks)
        if self.device_chunks and (self.device is None or self.device.type != "cuda"):
            raise ValueError("device_chunks=True needs a GPU device (device='cuda'): the chunks live in device memory")
        if device_chunk_bytes is not None and int(device_chunk_bytes) < 0:
            raise ValueError("device_chunk_bytes must not be negative")
        self.device_chunk_bytes = None if device_chunk_bytes is None else int(device_chunk_bytes)
        self._warned_budget = False
        # raw-count chunks (opt-in): see _tensor / _upload_chunk
        from . import preprocess

        if normalize is not None and normalize not in preprocess.NORMALIZE_MODES:
            raise ValueError(f"normalize must be None or one of {preprocess.NORMALIZE_MODES}, got {normalize!r}")
        self.normalize = normalize
        self.target_sum = preprocess.check_target_sum(target_sum)
        self._checked_raw = False

    def _check_raw(self, matrix, where: str) -> None:
        """Guard against normalising twice: once per object, the first stored values of the first chunk loaded are looked
        at on the host; anything but non-negative integers draws one RuntimeWarning."""
        if self.normalize is None or self._checked_raw:
            return
        self._checked_raw = True
        head = np.asarray(matrix.data[:min(len(matrix.data), 65536)])
        if head.size and bool(((head < 0) | (head != np.floor(head))).any()):
            warnings.warn(f"{where}: normalize={self.normalize!r} but the chunk does not look like raw counts (stored "
                          "values that are not non-negative integers): is it normalised already?", RuntimeWarning)

    # ---- chunks: (scipy CSR over the mapped file, metadata, row order)
    def _prepared_chunks(self, rng: np.random.Generator) -> Iterator:
        order = list(range(len(self.chunks)))
        if self.shuffle:
            order = [int(i) for i in rng.permutation(len(order))]
        for ci in order:
            matrix, metadata = load_chunk(*self.chunks[ci])
            self._check_raw(matrix, self.chunks[ci][0])
            rows = rng.permutation(matrix.shape[0]) if self.shuffle else np.arange(matrix.shape[0])
            yield matrix, metadata, rows.astype(np.int64)

    def _background(self, gen: Iterator) -> Iterator:
        """Run `gen` in a thread, one item ahead (loading a chunk overlaps the training on the last one).  The thread
        stops when the consumer is closed or collected."""
        q: "queue.Queue" = queue.Queue(maxsize=1)
        done, stop = object(), threading.Event()

        def put(item) -> bool:
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def work():
            try:
                for item in gen:
                    if not put(item):
                        return
                put(done)
            except BaseException as e:  # noqa: BLE001 -- re-raised in the consumer
                put(e)

        thread = threading.Thread(target=work, daemon=True)
        thread.start()
        _LIVE_PRODUCERS.append((stop, thread))
        try:
            while True:
                item = q.get()
                if item is done:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            stop.set()
            if _LIVE_PRODUCERS is not None and (stop, thread) in _LIVE_PRODUCERS:
                _LIVE_PRODUCERS.remove((stop, thread))

    # ---- one batch: native gather into a staging slot (worker thread), tensors + H2D (consumer thread)
    def _gather(self, slot: _Slot, matrix, rows: np.ndarray):
        lib = feed_lib()
        ib = matrix.indptr.dtype.itemsize
        if matrix.indices.dtype.itemsize != ib or ib not in (4, 8) or matrix.data.dtype != np.float32:
            matrix = matrix.astype(np.float32) if matrix.data.dtype != np.float32 else matrix
            matrix.indices = matrix.indices.astype(matrix.indptr.dtype)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        nnz = lib.mmvae_feed_rows_nnz(matrix.indptr.ctypes.data, ib, matrix.shape[0], rows.ctypes.data, len(rows))
        if nnz < 0:
            raise ValueError("row index outside the chunk")
        slot.reserve(nnz)
        got = C.c_int64(0)
        if slot.index_dtype == torch.int32 and matrix.shape[1] > 0x7fffffff:
            raise ValueError("a chunk with more than 2^31 - 1 columns needs index_dtype=torch.int64")
        fn = lib.mmvae_feed_gather_rows_i32 if slot.index_dtype == torch.int32 else lib.mmvae_feed_gather_rows
        rc = fn(matrix.indptr.ctypes.data, matrix.indices.ctypes.data if nnz else None, ib,
                matrix.data.ctypes.data if nnz else None, matrix.shape[0], rows.ctypes.data, len(rows), slot.crow.data_ptr(),
                slot.col.data_ptr(), slot.val.data_ptr(), max(slot.col.numel(), nnz), self.gather_threads, C.byref(got))
        if rc != 0 or got.value != nnz:
            raise RuntimeError(f"mmvae_feed_gather_rows failed with code {rc}")
        return slot, int(nnz), len(rows)

    def _tensor(self, slot: _Slot, nnz: int, n_rows: int, n_cols: int) -> torch.Tensor:
        """Staging slot -> torch.sparse_csr (int32 / int64 indices, fp32 values), on the device when one
        was given (three non-blocking copies out of page-locked memory; the slot is reusable once they are done)."""
        crow, col, val = slot.crow[:n_rows + 1], slot.col[:nnz], slot.val[:nnz]
        if self.device is not None and self.device.type == "cuda" and slot.packed:
            o_col, o_val, words = slot.layout(nnz)
            dev = slot.buf[:words].to(self.device, non_blocking=True)  # one copy; the three arrays are views of it
            crow, col, val = dev[:n_rows + 1], dev[o_col:o_col + nnz], dev[o_val:o_val + nnz].view(torch.float32)
            slot.event = torch.cuda.Event()
            slot.event.record()
        elif self.device is not None and self.device.type == "cuda":
            crow, col, val = (t.to(self.device, non_blocking=True) for t in (crow, col, val))
            slot.event = torch.cuda.Event()
            slot.event.record()
        else:  # host batches own their arrays: the slot was allocated for this batch alone (see __iter__)
            slot.crow, slot.col, slot.val = slot.crow.new_empty(0), slot.col.new_empty(0), slot.val.new_empty(0)
        if self.normalize is not None and n_rows:  # raw counts: normalised here, before the batch is densified
            if val.is_cuda:
                from . import ops

                ops.csr_log1p_normalize_(crow, val, self.target_sum)
            else:
                from . import preprocess

                preprocess._normalize_cpu(crow.numpy(), val.numpy(), self.target_sum)
        t = torch.sparse_csr_tensor(crow, col, val, size=(n_rows, n_cols))
        if self.return_dense:
            from . import backend

            t = backend.to_dense(t) if t.values().is_cuda else t.to_dense()
        return t

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, pd.DataFrame, str]]:
        from collections import deque

        if self.device_chunks:
            yield from self._iter_device()
            return
        rng = np.random.default_rng([self.seed, self.epoch])
        self.epoch += 1
        chunks = self._prepared_chunks(rng)
        if self.prefetch:
            chunks = self._background(chunks)
        pinned = self.device is not None and self.device.type == "cuda"
        depth = self.workers + 1
        if (len(self._slots) != depth or (self._slots and self._slots[0].pinned != pinned)
                or (self._slots and self._slots[0].index_dtype != self.index_dtype)):
            self._slots = [_Slot(self.batch_size, pinned, self.index_dtype) for _ in range(depth)]
        free = deque(self._slots)
        inflight: deque = deque()

        def jobs():
            dealt = []  # the current round of `world` consecutive kept batches of the epoch
            for matrix, metadata, order in chunks:
                n = matrix.shape[0]
                for i in range(0, n, self.batch_size):
                    if i + self.batch_size > n and not self.allow_partials:
                        continue
                    dealt.append((matrix, metadata, order[i:i + self.batch_size]))
                    if len(dealt) == self.world:
                        yield dealt[self.rank]
                        dealt = []

        with _Workers(self.workers) as pool:
            def finish():
                fut, matrix, metadata, rows = inflight.popleft()
                slot, nnz, n_rows = fut.result()
                x = self._tensor(slot, nnz, n_rows, matrix.shape[1])
                free.append(slot)
                # the batch's metadata rows under a fresh 0..n-1 index (cellxgene_datapipe.py:110-122 slices the permuted
                # frame): take + a new RangeIndex is half the cost of iloc + reset_index, same frame (tested)
                md = metadata.take(rows)
                md.index = pd.RangeIndex(len(md))
                return x, md, self.name

            for matrix, metadata, rows in jobs():
                if not free:
                    yield finish()
                slot = free.popleft()
                if not pinned:  # host batches keep the arrays they were gathered into
                    slot.crow = torch.empty(self.batch_size + 1, dtype=self.index_dtype)
                if slot.event is not None:  # the H2D copies that read this slot (depth batches ago) must be done
                    slot.event.synchronize()
                    slot.event = None
                inflight.append((pool.submit(self._gather, slot, matrix, rows), matrix, metadata, rows))
            while inflight:
                yield finish()

    # ---- device-resident chunks: one upload per chunk (chunk thread), one gather launch per batch (consumer thread)
    @staticmethod
    def _pad16(n: int) -> int:
        return (n + 15) // 16 * 16

    def _chunk_bytes(self, n_rows: int, nnz: int, n_batches: int) -> int:
        """Device bytes of a resident chunk: row pointers, column indices, values, row order and the batches' table."""
        isz = 4 if self.index_dtype == torch.int32 else 8
        return (self._pad16((n_rows + 1) * isz) + self._pad16(nnz * isz) + self._pad16(nnz * 4) + self._pad16(n_rows * 8)
                + self._pad16(n_batches * (self.batch_size + 1) * isz))

    def _upload_chunk(self, matrix, metadata, order: np.ndarray, where: str, stream, staging: dict) -> _DeviceChunk:
        """Canonical fp32 CSR in `index_dtype`, checked on the host, packed into page-locked staging and sent to the device
        by two non-blocking copies on `stream` (the chunk's arrays + row order; the small table of its batches, which the
        batches' `crow_indices` are views of and which therefore lives as long as the last of them)."""
        n, G = matrix.shape
        nnz = len(matrix.indices)
        if self.index_dtype == torch.int32 and (G > 0x7fffffff or nnz > 0x7fffffff):
            raise ValueError(f"{where}: a chunk with more than 2^31 - 1 columns or stored elements needs "
                             "index_dtype=torch.int64")
        validate_csr_chunk(matrix.indptr, matrix.indices, matrix.data, G, where)
        np_idx = np.int32 if self.index_dtype == torch.int32 else np.int64
        table, nnzs, n_rows = batch_row_pointers(matrix.indptr, order, self.batch_size, self.allow_partials, np_idx)
        isz = np.dtype(np_idx).itemsize
        parts = [(matrix.indptr, np_idx, self.index_dtype), (matrix.indices, np_idx, self.index_dtype),
                 (matrix.data, np.float32, torch.float32), (order, np.int64, torch.int64),
                 (table.reshape(-1), np_idx, self.index_dtype)]
        offsets, total = [], 0
        for src, np_dtype, _ in parts:
            offsets.append(total)
            total += self._pad16(len(src) * np.dtype(np_dtype).itemsize)
        o_table = offsets[-1]
        if staging.get("event") is not None:  # the copies that read the staging buffer (last chunk's) must be done
            staging["event"].synchronize()
            staging["event"] = None
        if staging.get("buf") is None or staging["buf"].numel() < total:
            staging["buf"] = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = staging["buf"].numpy()
        for (src, np_dtype, _), o in zip(parts, offsets):
            nb = len(src) * np.dtype(np_dtype).itemsize
            np.copyto(host[o:o + nb].view(np_dtype), src, casting="unsafe")  # (ranges checked above)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            buf = torch.empty(max(o_table, 16), dtype=torch.uint8, device=self.device)
            tbuf = torch.empty(max(total - o_table, 16), dtype=torch.uint8, device=self.device)
            if o_table:
                buf[:o_table].copy_(staging["buf"][:o_table], non_blocking=True)
            if total > o_table:
                tbuf[:total - o_table].copy_(staging["buf"][o_table:total], non_blocking=True)
            dev = []
            for (src, np_dtype, t_dtype), o in zip(parts[:4], offsets[:4]):
                dev.append(buf[o:o + len(src) * np.dtype(np_dtype).itemsize].view(t_dtype))
            csr = torch.sparse_csr_tensor(dev[0], dev[1], dev[2], size=(n, G))
            tab = tbuf[:table.size * isz].view(self.index_dtype).view(table.shape[0], self.batch_size + 1)
            if self.normalize is not None and n:  # raw counts: one launch behind the copies, ahead of the gathers' event
                from . import ops

                ops.csr_log1p_normalize_(dev[0], dev[2], self.target_sum, stream=stream)
            event = torch.cuda.Event()
            event.record(stream)
        staging["event"] = event
        return _DeviceChunk((buf, tbuf), csr, dev[3], tab, nnzs, n_rows, event, metadata, order)

    def _device_chunks(self, rng: np.random.Generator, budget: int, resident: threading.Semaphore,
                       stop: threading.Event) -> Iterator:
        """`_prepared_chunks` (same generator calls in the same order) whose chunks go to the device as they are loaded:
        yields `_DeviceChunk`s, or `(matrix, metadata, rows)` for a chunk over the budget (host path for that chunk).
        Holds one of the two `resident` permits per uploaded chunk; the consumer gives it back when it is done with it."""
        order = list(range(len(self.chunks)))
        if self.shuffle:
            order = [int(i) for i in rng.permutation(len(order))]
        stream = torch.cuda.Stream(device=self.device)
        staging: dict = {}
        for ci in order:
            where = self.chunks[ci][0]
            matrix, metadata = load_chunk(*self.chunks[ci])
            self._check_raw(matrix, where)
            n = matrix.shape[0]
            rows = (rng.permutation(n) if self.shuffle else np.arange(n)).astype(np.int64)
            n_batches = -(-n // self.batch_size) if self.allow_partials else n // self.batch_size
            if n_batches == 0:
                continue
            need = self._chunk_bytes(n, len(matrix.indices), n_batches)
            if need > budget:
                if not self._warned_budget:
                    self._warned_budget = True
                    warnings.warn(f"{where}: the chunk needs {need} bytes of device memory, over device_chunk_bytes = "
                                  f"{budget}: chunks over the budget are gathered on the host", RuntimeWarning)
                yield matrix, metadata, rows
                continue
            while not resident.acquire(timeout=0.1):
                if stop.is_set():
                    return
            yield self._upload_chunk(matrix, metadata, rows, where, stream, staging)
        if staging.get("event") is not None:
            staging["event"].synchronize()

    def _device_batch(self, ch: _DeviceChunk, k: int):
        """Batch k of a resident chunk: one gather launch on the current (producing) stream + the metadata slice."""
        from . import ops

        cur = torch.cuda.current_stream(self.device)
        if ch.ready != cur.cuda_stream:  # once per chunk: behind the upload; the chunk must outlive this stream's gathers
            cur.wait_event(ch.event)
            for b in ch.buf:
                b.record_stream(cur)
            ch.ready = cur.cuda_stream
        B, n_rows = self.batch_size, ch.n_rows[k]
        rows = ch.rows[k * B:k * B + n_rows]
        if self.return_dense:
            x = ops.csr_gather_rows_dense(ch.csr, rows)
        else:
            x = ops.csr_gather_rows(ch.csr, rows, ch.table[k, :n_rows + 1], ch.nnz[k])
        md = ch.metadata.take(ch.order[k * B:k * B + n_rows])
        md.index = pd.RangeIndex(len(md))
        return x, md, self.name

    def _host_batch(self, slots: list, matrix, metadata, rows: np.ndarray):
        """One batch of a chunk over the device budget: the host gather and staging of `__iter__`, made in line."""
        slot = slots.pop(0)
        slots.append(slot)
        if slot.event is not None:
            slot.event.synchronize()
            slot.event = None
        slot, nnz, n_rows = self._gather(slot, matrix, rows)
        x = self._tensor(slot, nnz, n_rows, matrix.shape[1])
        md = metadata.take(rows)
        md.index = pd.RangeIndex(len(md))
        return x, md, self.name

    def _iter_device(self) -> Iterator[Tuple[torch.Tensor, pd.DataFrame, str]]:
        """`__iter__` with device-resident chunks.  Same chunk order, row orders, batches and dealing among ranks; the
        batch dealt to this rank is gathered when its turn comes and handed out once its round of `world` is complete."""
        rng = np.random.default_rng([self.seed, self.epoch])
        self.epoch += 1
        budget = self.device_chunk_bytes
        if budget is None:
            budget = torch.cuda.mem_get_info(self.device)[0] // 4
        resident, stop = threading.Semaphore(2), threading.Event()
        chunks = self._device_chunks(rng, budget, resident, stop)
        if self.prefetch:
            chunks = self._background(chunks)
        slots: list = []
        dealt, mine = 0, None
        B = self.batch_size
        try:
            for item in chunks:
                ch = item if isinstance(item, _DeviceChunk) else None
                if ch is None:
                    matrix, metadata, order = item
                    if not slots:
                        slots = [_Slot(B, True, self.index_dtype) for _ in range(2)]
                    n = matrix.shape[0]
                    starts = [i for i in range(0, n, B) if i + B <= n or self.allow_partials]
                item = None
                try:
                    for k in (range(len(ch.nnz)) if ch is not None else range(len(starts))):
                        if dealt == self.rank:
                            mine = (self._device_batch(ch, k) if ch is not None
                                    else self._host_batch(slots, matrix, metadata, order[starts[k]:starts[k] + B]))
                        dealt += 1
                        if dealt == self.world:
                            dealt = 0
                            out, mine = mine, None
                            yield out
                finally:
                    if ch is not None:
                        ch = None
                        resident.release()
        finally:
            stop.set()
            chunks.close()

    def __len__(self) -> int:
        raise TypeError("SpeciesChunks streams chunk files: its length is not known without reading them")


_LIVE_PRODUCERS: list = []  # (stop event, thread) of running Prefetcher producers, stopped and joined at interpreter exit


def _stop_producers() -> None:
    """A daemon thread that is still inside torch when the interpreter finalises is torn down by a forced unwind through
    C++ frames (`terminate called without an active exception`): stop and join the producers first."""
    for stop, thread in list(_LIVE_PRODUCERS):
        stop.set()
    for stop, thread in list(_LIVE_PRODUCERS):
        thread.join(timeout=10.0)
    _LIVE_PRODUCERS.clear()


atexit.register(_stop_producers)
if hasattr(threading, "_register_atexit"):  # also before the interpreter starts joining threads
    threading._register_atexit(_stop_producers)


class Prefetcher:
    """Runs a batch iterable -- `SpeciesChunks`, `trainer.MultiModalBatches` over several of them -- in a background
    thread, `depth` batches ahead of the training loop, so that the consumer thread only launches steps: waiting for a
    gather, slicing the metadata and enqueueing the host-to-device copies no longer sit between two step launches.
    On a GPU the producer issues its copies on a stream of its own; the consumer's stream waits for the event recorded
    behind each batch, and the batch's device arrays are marked as used by the consumer's stream (allocator safety).
    Order and content of the batches are unchanged; an exception in the producer is re-raised in the consumer."""

    def __init__(self, batches, depth: int = 3, device: Optional[Union[str, torch.device]] = None):
        self.batches = batches
        self.depth = max(1, int(depth))
        self.device = torch.device(device) if device is not None else None

    def __iter__(self):
        from contextlib import nullcontext

        q: "queue.Queue" = queue.Queue(maxsize=self.depth)
        done, stop = object(), threading.Event()
        on_gpu = self.device is not None and self.device.type == "cuda"
        stream = torch.cuda.Stream(device=self.device) if on_gpu else None

        def put(item) -> bool:
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def work():
            try:
                with (torch.cuda.stream(stream) if on_gpu else nullcontext()):
                    source = iter(self.batches)
                    while True:
                        try:
                            item = next(source)
                        except StopIteration:
                            break
                        ev = None
                        if on_gpu:
                            ev = torch.cuda.Event()
                            ev.record(stream)
                        if not put((item, ev)):
                            return
                put(done)
            except BaseException as e:  # noqa: BLE001 -- re-raised in the consumer
                put(e)

        thread = threading.Thread(target=work, daemon=True)
        thread.start()
        entry = (stop, thread)
        _LIVE_PRODUCERS.append(entry)
        try:
            while True:
                got = q.get()
                if got is done:
                    return
                if isinstance(got, BaseException):
                    raise got
                item, ev = got
                if ev is not None:
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(ev)
                    x = item[0] if isinstance(item, tuple) else item
                    if torch.is_tensor(x) and x.is_cuda:
                        parts = ((x.crow_indices(), x.col_indices(), x.values()) if x.layout == torch.sparse_csr else (x,))
                        for part in parts:
                            part.record_stream(cur)
                yield item
        finally:
            stop.set()
            if _LIVE_PRODUCERS is not None and entry in _LIVE_PRODUCERS:  # (None: the interpreter is shutting down)
                _LIVE_PRODUCERS.remove(entry)


def write_chunks(directory: str, name: str, matrix, metadata: pd.DataFrame, chunk_rows: int, split: str = "train",
                 compressed: bool = True) -> List[str]:
    """Write `{name}_{split}_counts_{i}.npz` / `{name}_{split}_metadata_{i}.pkl` chunk pairs (the layout the
    reference's preprocessing produces, scripts/data-preprocessing/: `scipy.sparse.save_npz` + pickled DataFrame).
    Used by the tests and by bench.py's npz leg to put synthetic data on disk."""
    import scipy.sparse as sp

    os.makedirs(directory, exist_ok=True)
    matrix = sp.csr_matrix(matrix)
    out = []
    for k, i in enumerate(range(0, matrix.shape[0], chunk_rows), start=1):
        npz = os.path.join(directory, f"{name}_{split}_counts_{k}.npz")
        pkl = os.path.join(directory, f"{name}_{split}_metadata_{k}.pkl")
        sp.save_npz(npz, matrix[i:i + chunk_rows], compressed=compressed)
        metadata.iloc[i:i + chunk_rows].reset_index(drop=True).to_pickle(pkl)
        out += [npz, pkl]
    return out
