"""ctypes binding of libmmvae_hist.so (the C-ABI declared in include/mmvae_hist.h): segmented histograms of a flat fp32
array -- one pass over an optimiser's gradient arena gives every parameter's histogram.

The fifth device library beside libmmvae_hip.so, libmmvae_stats.so, libmmvae_disc.so and libmmvae_umap.so, with its own
version counter, so that it does not move the training step's ABI.  Like `_lib`, it is the product: missing or
unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

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

BINDING = Binding("libmmvae_hist.so", "mmvae_hist.h", HIST_PROTOTYPES, "mmvae_hist_abi_version", HIST_ABI_VERSION,
                  "mmvae_hist_build_arch")
HIST_LIB_PATH = BINDING.path

_hist: Optional[C.CDLL] = None


def load_hist() -> C.CDLL:
    """Load libmmvae_hist.so (see _bind.Binding.load).  Raises loudly."""
    global _hist
    if _hist is not None:
        return _hist
    _hist = BINDING.load()
    return _hist
