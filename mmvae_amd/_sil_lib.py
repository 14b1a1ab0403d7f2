"""ctypes binding of libmmvae_sil.so (the C-ABI declared in include/mmvae_sil.h): silhouette widths of latent embeddings
-- per cell, the mean distance to its own class against the nearest other class of its group, over all cells.

A satellite device library with its own version counter, so that it moves neither the training step's ABI nor the UMAP
library's.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

SIL_ABI_VERSION = 1
SIL_MAX_D = 512
SIL_EUCLIDEAN = 0
SIL_COSINE = 1

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64

# name -> (restype, argtypes), in the order of include/mmvae_sil.h (tests/test_silhouette_host.py checks that every symbol
# the header declares is listed here and exported by the .so)
SIL_PROTOTYPES = {
    "mmvae_sil_abi_version": (_i, []),
    "mmvae_sil_build_arch": (C.c_char_p, []),
    "mmvae_sil_rows_workspace_bytes": (C.c_size_t, [_i, _i]),
    "mmvae_sil_rows_f32": (_i, [_i, _i, _p, _l, _i, _i, _p, _p, _p, _p, _p, _p, _p, C.c_size_t, _p]),
}

BINDING = Binding("libmmvae_sil.so", "mmvae_sil.h", SIL_PROTOTYPES, "mmvae_sil_abi_version", SIL_ABI_VERSION,
                  "mmvae_sil_build_arch")
SIL_LIB_PATH = BINDING.path

_sil: Optional[C.CDLL] = None


def load_sil() -> C.CDLL:
    """Load libmmvae_sil.so (see _bind.Binding.load).  Raises loudly."""
    global _sil
    if _sil is not None:
        return _sil
    _sil = BINDING.load()
    return _sil
