"""ctypes binding of libmmvae_hist.so (the C-ABI declared in include/mmvae_hist.h): segmented histograms of a flat fp32
array -- one pass over an optimiser's gradient arena gives every parameter's histogram.

The fifth device library beside libmmvae_hip.so, libmmvae_stats.so, libmmvae_disc.so and libmmvae_umap.so, with its own
version counter, so that it does not move the training step's ABI.  Like `_lib`, it is the product: missing or
unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

_HERE = os.path.dirname(os.path.abspath(__file__))
HIST_LIB_PATH = os.path.join(_HERE, "csrc", "libmmvae_hist.so")

HIST_ABI_VERSION = 1
HIST_ITEM_ELEMS = 8192
HIST_MAX_EDGES = 2048
HIST_STATS = 8
# the fields of a stats row, in order (the enum of include/mmvae_hist.h)
HIST_STAT_NAMES = ("min", "max", "num_finite", "sum", "sum_squares", "n_nonfinite", "n_below", "n_above")
# struct mmvae_hist_item as a numpy structured dtype
HIST_ITEM_DTYPE = [("offset", "<i8"), ("len", "<i4"), ("segment", "<i4")]

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_z = C.c_size_t
_f = C.c_float

# name -> (restype, argtypes), in the order of include/mmvae_hist.h (tests/test_grad_hist_host.py checks that every symbol
# the header declares is listed here and exported by the .so)
HIST_PROTOTYPES = {
    "mmvae_hist_abi_version": (_i, []),
    "mmvae_hist_build_arch": (C.c_char_p, []),
    "mmvae_hist_workspace_bytes": (_z, [_l, _i, _i]),
    "mmvae_hist_segments_f32": (_i, [_l, _p, _i, _p, _f, _i, _p, _p, _p, _p, _z, _p]),
}

_hist: Optional[C.CDLL] = None


def load_hist() -> C.CDLL:
    """Load libmmvae_hist.so (built by __graft_entry__.build() / `make -C mmvae_amd/csrc`).  Raises loudly."""
    global _hist
    if _hist is not None:
        return _hist
    import torch  # noqa: F401  (torch's HIP runtime must be the process's: see _lib.load)

    if not os.path.exists(HIST_LIB_PATH):
        raise HipLibraryError(
            f"{HIST_LIB_PATH} not found: build it with `make -C mmvae_amd/csrc` (or __graft_entry__.build()). "
            "mmvae_amd has no non-HIP execution path for device tensors."
        )
    try:
        lib = C.CDLL(HIST_LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"could not load {HIST_LIB_PATH}: {e}") from e
    for name, (res, args) in HIST_PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{HIST_LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.mmvae_hist_abi_version() != HIST_ABI_VERSION:
        raise HipLibraryError(f"{HIST_LIB_PATH} has ABI {lib.mmvae_hist_abi_version()}, this binding was written "
                              f"against {HIST_ABI_VERSION}: rebuild it")
    _hist = lib
    return lib
