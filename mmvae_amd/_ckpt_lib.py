"""ctypes binding of libmmvae_ckpt.so (the C-ABI declared in include/mmvae_ckpt.h): the device snapshot behind a
checkpoint -- one launch that copies a table of ranges into a private buffer and computes, per range, a 64-bit checksum
and a count of non-finite values.

The eighth device library beside libmmvae_hip.so, libmmvae_stats.so, libmmvae_disc.so, libmmvae_umap.so,
libmmvae_hist.so, libmmvae_prep.so and libmmvae_plot.so, with its own version counter, so that it does not move the
training step's ABI.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

CKPT_ABI_VERSION = 1
CKPT_F32 = 1
CKPT_CHUNK_WORDS = 8192
CKPT_MAX_GROUPS = 2048

_p = C.c_void_p
_i = C.c_int
_u = C.c_uint64


class CkptJob(C.Structure):
    """mmvae_ckpt_job (32 bytes)."""
    _fields_ = [("src", _p), ("dst_word", _u), ("n_words", _u), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# the same record as a numpy structured dtype (tables are built with numpy and uploaded as bytes)
JOB_DTYPE = [("src", "<u8"), ("dst_word", "<u8"), ("n_words", "<u8"), ("flags", "<u4"), ("reserved", "<u4")]

# name -> (restype, argtypes), in the order of include/mmvae_ckpt.h (tests/test_checkpoint_host.py checks that every symbol
# the header declares is listed here and exported by the .so)
CKPT_PROTOTYPES = {
    "mmvae_ckpt_abi_version": (_i, []),
    "mmvae_ckpt_build_arch": (C.c_char_p, []),
    "mmvae_ckpt_check_jobs": (_i, [_i, _p, C.POINTER(_u)]),
    "mmvae_ckpt_snapshot": (_i, [_i, _p, _u, _p, _p, _p]),
}

BINDING = Binding("libmmvae_ckpt.so", "mmvae_ckpt.h", CKPT_PROTOTYPES, "mmvae_ckpt_abi_version", CKPT_ABI_VERSION,
                  "mmvae_ckpt_build_arch")
CKPT_LIB_PATH = BINDING.path

_ckpt: Optional[C.CDLL] = None


def load_ckpt() -> C.CDLL:
    """Load libmmvae_ckpt.so (see _bind.Binding.load).  Raises loudly."""
    global _ckpt
    if _ckpt is not None:
        return _ckpt
    _ckpt = BINDING.load()
    return _ckpt
