"""ctypes binding of libmmvae_prep.so (the C-ABI declared in include/mmvae_prep.h): log1p-per-10k normalisation of a raw
CSR count chunk where it lies in device memory, with the per-cell totals as a by-product.

The sixth device library beside libmmvae_hip.so, libmmvae_stats.so, libmmvae_disc.so, libmmvae_umap.so and
libmmvae_hist.so, with its own version counter, so that it does not move the training step's ABI.  Like `_lib`, it is the
product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

PREP_ABI_VERSION = 1
PREP_ROWS_PER_GROUP = 4
PREP_REG_ELEMS = 1024

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_f = C.c_float

_NORM = (_i, [_l, _l, _p, _p, _f, _p, _p])
# name -> (restype, argtypes), in the order of include/mmvae_prep.h (tests/test_prep_host.py checks that every symbol the
# header declares is listed here and exported by the .so)
PREP_PROTOTYPES = {
    "mmvae_prep_abi_version": (_i, []),
    "mmvae_prep_build_arch": (C.c_char_p, []),
    "mmvae_prep_csr_log1p_norm_i32": _NORM,
    "mmvae_prep_csr_log1p_norm_i64": _NORM,
}

BINDING = Binding("libmmvae_prep.so", "mmvae_prep.h", PREP_PROTOTYPES, "mmvae_prep_abi_version", PREP_ABI_VERSION,
                  "mmvae_prep_build_arch")
PREP_LIB_PATH = BINDING.path

_prep: Optional[C.CDLL] = None


def load_prep() -> C.CDLL:
    """Load libmmvae_prep.so (see _bind.Binding.load).  Raises loudly."""
    global _prep
    if _prep is not None:
        return _prep
    _prep = BINDING.load()
    return _prep
