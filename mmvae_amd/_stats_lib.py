"""ctypes binding of libmmvae_stats.so (the C-ABI declared in include/mmvae_stats.h): evaluation statistics.

A library of its own beside libmmvae_hip.so, with its own version counter, so that a new statistic does not move the
training step's ABI.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

STATS_ABI_VERSION = 1
ROW_CORR_MAX_ROWS = 2048
ROW_CORR_STATS = 8

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_z = C.c_size_t

# name -> (restype, argtypes), in the order of include/mmvae_stats.h (tests/test_cell_correlation_host.py checks that
# every symbol the header declares is listed here and exported by the .so)
STATS_PROTOTYPES = {
    "mmvae_stats_abi_version": (_i, []),
    "mmvae_stats_build_arch": (C.c_char_p, []),
    "mmvae_stats_row_corr_workspace_bytes": (_z, [_i, _i, _i]),
    "mmvae_stats_row_corr_f32": (_i, [_i, _i, _i, _p, _l, _p, _l, _p, _l, _p, _p, _z, _p]),
}

BINDING = Binding("libmmvae_stats.so", "mmvae_stats.h", STATS_PROTOTYPES, "mmvae_stats_abi_version", STATS_ABI_VERSION,
                  "mmvae_stats_build_arch")
STATS_LIB_PATH = BINDING.path

_stats: Optional[C.CDLL] = None


def load_stats() -> C.CDLL:
    """Load libmmvae_stats.so (see _bind.Binding.load).  Raises loudly."""
    global _stats
    if _stats is not None:
        return _stats
    _stats = BINDING.load()
    return _stats
