"""ctypes binding of libmmvae_umap.so (the C-ABI declared in include/mmvae_umap.h): the UMAP of latent embeddings.

The fourth device library beside libmmvae_hip.so, libmmvae_stats.so and libmmvae_disc.so, with its own version counter,
so that it does not move the training step's ABI.  Like `_lib`, it is the product: missing or unloadable, every call
raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

UMAP_ABI_VERSION = 1
UMAP_MAX_K = 64
UMAP_MAX_D = 512

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_u = C.c_uint64
_z = C.c_size_t
_f = C.c_float

# name -> (restype, argtypes), in the order of include/mmvae_umap.h (tests/test_umap_host.py checks that every symbol the
# header declares is listed here and exported by the .so)
UMAP_PROTOTYPES = {
    "mmvae_umap_abi_version": (_i, []),
    "mmvae_umap_build_arch": (C.c_char_p, []),
    "mmvae_umap_knn_cosine_workspace_bytes": (_z, [_i, _i, _i]),
    "mmvae_umap_knn_cosine_f32": (_i, [_i, _i, _i, _p, _l, _p, _p, _p, _z, _p]),
    "mmvae_umap_smooth_knn_f32": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "mmvae_umap_random_init_f32": (_i, [_l, _p, _u, _p]),
    "mmvae_umap_layout_f32": (_i, [_i, _i, _p, _p, _p, _p, _p, _f, _f, _f, _i, _i, _i, _u, _p]),
}

BINDING = Binding("libmmvae_umap.so", "mmvae_umap.h", UMAP_PROTOTYPES, "mmvae_umap_abi_version", UMAP_ABI_VERSION,
                  "mmvae_umap_build_arch")
UMAP_LIB_PATH = BINDING.path

_umap: Optional[C.CDLL] = None


def load_umap() -> C.CDLL:
    """Load libmmvae_umap.so (see _bind.Binding.load).  Raises loudly."""
    global _umap
    if _umap is not None:
        return _umap
    _umap = BINDING.load()
    return _umap
