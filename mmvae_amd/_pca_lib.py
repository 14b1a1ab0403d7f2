"""ctypes binding of libmmvae_pca.so (the C-ABI declared in include/mmvae_pca.h): the per-class column sums, the centred
scatter matrix and the projection on the components that a PCA of latent embeddings and the principal-component
regression of a covariate need.

A satellite device library with its own version counter, so that it moves neither the training step's ABI nor another
satellite's.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

PCA_ABI_VERSION = 1
PCA_MAX_D = 512
PCA_MAX_COV = 8
PCA_CHAIN = 256
PCA_SEGMENT = 256
PCA_PARTIAL_CAP = 64 << 20
PCA_MAX_SUMS = 1 << 30

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_z = C.c_size_t

# name -> (restype, argtypes), in the order of include/mmvae_pca.h (tests/test_pcr_host.py checks that every symbol the
# header declares is listed here and exported by the .so)
PCA_PROTOTYPES = {
    "mmvae_pca_abi_version": (_i, []),
    "mmvae_pca_build_arch": (C.c_char_p, []),
    "mmvae_pca_group_sums_workspace_bytes": (_z, [_i, _i]),
    "mmvae_pca_group_sums_f64": (_i, [_i, _i, _p, _l, _p, _i, _p, _p, _p, _p, _z, _p]),
    "mmvae_pca_scatter_workspace_bytes": (_z, [_i, _i, _i]),
    "mmvae_pca_scatter_f32": (_i, [_i, _i, _p, _l, _i, _p, _l, _p, _p, _p, _z, _p]),
    "mmvae_pca_project_f32": (_i, [_i, _i, _p, _l, _p, _i, _p, _p, _l, _p]),
}

BINDING = Binding("libmmvae_pca.so", "mmvae_pca.h", PCA_PROTOTYPES, "mmvae_pca_abi_version", PCA_ABI_VERSION,
                  "mmvae_pca_build_arch")
PCA_LIB_PATH = BINDING.path

_pca: Optional[C.CDLL] = None


def load_pca() -> C.CDLL:
    """Load libmmvae_pca.so (see _bind.Binding.load).  Raises loudly."""
    global _pca
    if _pca is not None:
        return _pca
    _pca = BINDING.load()
    return _pca
