"""ctypes binding of libmmvae_stats.so (the C-ABI declared in include/mmvae_stats.h): evaluation statistics.

A library of its own beside libmmvae_hip.so, with its own version counter, so that a new statistic does not move the
training step's ABI.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

_HERE = os.path.dirname(os.path.abspath(__file__))
STATS_LIB_PATH = os.path.join(_HERE, "csrc", "libmmvae_stats.so")

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

_stats: Optional[C.CDLL] = None


def load_stats() -> C.CDLL:
    """Load libmmvae_stats.so (built by __graft_entry__.build() / `make -C mmvae_amd/csrc`).  Raises loudly."""
    global _stats
    if _stats is not None:
        return _stats
    import torch  # noqa: F401  (torch's HIP runtime must be the process's: see _lib.load)

    if not os.path.exists(STATS_LIB_PATH):
        raise HipLibraryError(
            f"{STATS_LIB_PATH} not found: build it with `make -C mmvae_amd/csrc` (or __graft_entry__.build()). "
            "mmvae_amd has no non-HIP execution path for device tensors."
        )
    try:
        lib = C.CDLL(STATS_LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"could not load {STATS_LIB_PATH}: {e}") from e
    for name, (res, args) in STATS_PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{STATS_LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.mmvae_stats_abi_version() != STATS_ABI_VERSION:
        raise HipLibraryError(f"{STATS_LIB_PATH} has ABI {lib.mmvae_stats_abi_version()}, this binding was written "
                              f"against {STATS_ABI_VERSION}: rebuild it")
    _stats = lib
    return lib
