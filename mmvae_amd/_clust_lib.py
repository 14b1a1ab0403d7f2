"""ctypes binding of libmmvae_clust.so (the C-ABI declared in include/mmvae_clust.h): k-means on latent embeddings -- one
whole Lloyd iteration per call, and the distance pass of the k-means++ seeding.

A satellite device library with its own version counter, so that it moves neither the training step's ABI nor any other
satellite's.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

CLUST_ABI_VERSION = 1
CLUST_MAX_D = 512
CLUST_MAX_C = 256
CLUST_STATS_BYTES = 24  # { double inertia; double shift2; int32 changed; int32 empty; }

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64

# name -> (restype, argtypes), in the order of include/mmvae_clust.h (tests/test_clustering_host.py checks that every
# symbol the header declares is listed here and exported by the .so)
CLUST_PROTOTYPES = {
    "mmvae_clust_abi_version": (_i, []),
    "mmvae_clust_build_arch": (C.c_char_p, []),
    "mmvae_clust_kmeans_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "mmvae_clust_kmeans_step_f32": (_i, [_i, _i, _p, _l, _i, _p, _p, _p, _p, _p, _p, _p, C.c_size_t, _p]),
    "mmvae_clust_seed_update_f32": (_i, [_i, _i, _p, _l, _i, _i, _p, _p]),
}

BINDING = Binding("libmmvae_clust.so", "mmvae_clust.h", CLUST_PROTOTYPES, "mmvae_clust_abi_version", CLUST_ABI_VERSION,
                  "mmvae_clust_build_arch")
CLUST_LIB_PATH = BINDING.path

_clust: Optional[C.CDLL] = None


def load_clust() -> C.CDLL:
    """Load libmmvae_clust.so (see _bind.Binding.load).  Raises loudly."""
    global _clust
    if _clust is not None:
        return _clust
    _clust = BINDING.load()
    return _clust
