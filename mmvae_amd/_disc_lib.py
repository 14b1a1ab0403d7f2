"""ctypes binding of libmmvae_disc.so (the C-ABI declared in include/mmvae_disc.h): the meta-discriminators.

The third library, beside libmmvae_hip.so and libmmvae_stats.so, with its own version counter.  Like `_lib`, it is the
product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

_HERE = os.path.dirname(os.path.abspath(__file__))
DISC_LIB_PATH = os.path.join(_HERE, "csrc", "libmmvae_disc.so")

DISC_ABI_VERSION = 1
DISC_MAX_H1 = 256
DISC_MAX_H2 = 128
DISC_MAX_W2 = 16384
DISC_TILE_ROWS = 16
DISC_GRID_CAP = 128

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_z = C.c_size_t

# name -> (restype, argtypes), in the order of include/mmvae_disc.h (tests/test_meta_disc_host.py checks that every
# symbol the header declares is listed here and exported by the .so)
DISC_PROTOTYPES = {
    "mmvae_disc_abi_version": (_i, []),
    "mmvae_disc_build_arch": (C.c_char_p, []),
    "mmvae_disc_tail_workspace_bytes": (_z, [_i, _i, _i]),
    "mmvae_disc_tail_f32": (_i, [_i, _i, _i, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _z, _p]),
}

_disc: Optional[C.CDLL] = None


def load_disc() -> C.CDLL:
    """Load libmmvae_disc.so (built by __graft_entry__.build() / `make -C mmvae_amd/csrc`).  Raises loudly."""
    global _disc
    if _disc is not None:
        return _disc
    import torch  # noqa: F401  (torch's HIP runtime must be the process's: see _lib.load)

    if not os.path.exists(DISC_LIB_PATH):
        raise HipLibraryError(
            f"{DISC_LIB_PATH} not found: build it with `make -C mmvae_amd/csrc` (or __graft_entry__.build()). "
            "mmvae_amd has no non-HIP execution path for device tensors."
        )
    try:
        lib = C.CDLL(DISC_LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"could not load {DISC_LIB_PATH}: {e}") from e
    for name, (res, args) in DISC_PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{DISC_LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.mmvae_disc_abi_version() != DISC_ABI_VERSION:
        raise HipLibraryError(f"{DISC_LIB_PATH} has ABI {lib.mmvae_disc_abi_version()}, this binding was written "
                              f"against {DISC_ABI_VERSION}: rebuild it")
    _disc = lib
    return lib
