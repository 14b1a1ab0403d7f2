"""ctypes binding of libmmvae_umap.so (the C-ABI declared in include/mmvae_umap.h): the UMAP of latent embeddings.

The fourth device library beside libmmvae_hip.so, libmmvae_stats.so and libmmvae_disc.so, with its own version counter,
so that it does not move the training step's ABI.  Like `_lib`, it is the product: missing or unloadable, every call
raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

_HERE = os.path.dirname(os.path.abspath(__file__))
UMAP_LIB_PATH = os.path.join(_HERE, "csrc", "libmmvae_umap.so")

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

_umap: Optional[C.CDLL] = None


def load_umap() -> C.CDLL:
    """Load libmmvae_umap.so (built by __graft_entry__.build() / `make -C mmvae_amd/csrc`).  Raises loudly."""
    global _umap
    if _umap is not None:
        return _umap
    import torch  # noqa: F401  (torch's HIP runtime must be the process's: see _lib.load)

    if not os.path.exists(UMAP_LIB_PATH):
        raise HipLibraryError(
            f"{UMAP_LIB_PATH} not found: build it with `make -C mmvae_amd/csrc` (or __graft_entry__.build()). "
            "mmvae_amd has no non-HIP execution path for device tensors."
        )
    try:
        lib = C.CDLL(UMAP_LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"could not load {UMAP_LIB_PATH}: {e}") from e
    for name, (res, args) in UMAP_PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{UMAP_LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.mmvae_umap_abi_version() != UMAP_ABI_VERSION:
        raise HipLibraryError(f"{UMAP_LIB_PATH} has ABI {lib.mmvae_umap_abi_version()}, this binding was written "
                              f"against {UMAP_ABI_VERSION}: rebuild it")
    _umap = lib
    return lib
