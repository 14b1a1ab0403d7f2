"""ctypes binding of libmmvae_disc.so (the C-ABI declared in include/mmvae_disc.h): the meta-discriminators.

The third library, beside libmmvae_hip.so and libmmvae_stats.so, with its own version counter.  Like `_lib`, it is the
product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

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

BINDING = Binding("libmmvae_disc.so", "mmvae_disc.h", DISC_PROTOTYPES, "mmvae_disc_abi_version", DISC_ABI_VERSION,
                  "mmvae_disc_build_arch")
DISC_LIB_PATH = BINDING.path

_disc: Optional[C.CDLL] = None


def load_disc() -> C.CDLL:
    """Load libmmvae_disc.so (see _bind.Binding.load).  Raises loudly."""
    global _disc
    if _disc is not None:
        return _disc
    _disc = BINDING.load()
    return _disc
