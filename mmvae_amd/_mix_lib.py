"""ctypes binding of libmmvae_mix.so (the C-ABI declared in include/mmvae_mix.h): integration metrics on the latent kNN
graph -- the LISI calibration, LISI of code columns, and the label transfer from the other batches.

A satellite device library with its own version counter, so that it moves neither the training step's ABI nor the UMAP
library's.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

MIX_ABI_VERSION = 1
MIX_MAX_K = 64
MIX_MAX_COLS = 8

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_d = C.c_double

# name -> (restype, argtypes), in the order of include/mmvae_mix.h (tests/test_mixing_host.py checks that every symbol the
# header declares is listed here and exported by the .so)
MIX_PROTOTYPES = {
    "mmvae_mix_abi_version": (_i, []),
    "mmvae_mix_build_arch": (C.c_char_p, []),
    "mmvae_mix_calibrate_f32": (_i, [_i, _i, _p, _p, _d, _p, _p, _p]),
    "mmvae_mix_lisi_f32": (_i, [_i, _i, _p, _p, _p, _i, _p, _l, _p, _l, _p]),
    "mmvae_mix_transfer_f32": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
}

BINDING = Binding("libmmvae_mix.so", "mmvae_mix.h", MIX_PROTOTYPES, "mmvae_mix_abi_version", MIX_ABI_VERSION,
                  "mmvae_mix_build_arch")
MIX_LIB_PATH = BINDING.path

_mix: Optional[C.CDLL] = None


def load_mix() -> C.CDLL:
    """Load libmmvae_mix.so (see _bind.Binding.load).  Raises loudly."""
    global _mix
    if _mix is not None:
        return _mix
    _mix = BINDING.load()
    return _mix
