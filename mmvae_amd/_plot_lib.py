"""ctypes binding of libmmvae_plot.so (the C-ABI declared in include/mmvae_plot.h): per-pixel, per-class point counts of
an embedding and their composite into an RGBA8 picture.

The seventh device library beside libmmvae_hip.so, libmmvae_stats.so, libmmvae_disc.so, libmmvae_umap.so,
libmmvae_hist.so and libmmvae_prep.so, with its own version counter, so that it does not move the training step's ABI.
Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

PLOT_ABI_VERSION = 1
PLOT_MAX_CLASSES = 16
PLOT_MAX_MARKER = 8
PLOT_MAX_SIDE = 8192
# `mode` of mmvae_plot_count_f32
PLOT_COUNT_DEFAULT, PLOT_COUNT_PLAIN, PLOT_COUNT_AGGREGATE = 0, 1, 2

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_f = C.c_float

# name -> (restype, argtypes), in the order of include/mmvae_plot.h (tests/test_umap_plot_host.py checks that every symbol
# the header declares is listed here and exported by the .so)
PLOT_PROTOTYPES = {
    "mmvae_plot_abi_version": (_i, []),
    "mmvae_plot_build_arch": (C.c_char_p, []),
    "mmvae_plot_count_f32": (_i, [_l, _i, _p, _l, _p, _i, _i, _i, _i, C.POINTER(C.c_float), _i, _p, _p]),
    "mmvae_plot_composite_u8": (_i, [_p, _i, _i, _i, _p, _f, _f, _f, _f, _p, _p]),
}

BINDING = Binding("libmmvae_plot.so", "mmvae_plot.h", PLOT_PROTOTYPES, "mmvae_plot_abi_version", PLOT_ABI_VERSION,
                  "mmvae_plot_build_arch")
PLOT_LIB_PATH = BINDING.path

_plot: Optional[C.CDLL] = None


def load_plot() -> C.CDLL:
    """Load libmmvae_plot.so (see _bind.Binding.load).  Raises loudly."""
    global _plot
    if _plot is not None:
        return _plot
    _plot = BINDING.load()
    return _plot


def view_words(view) -> "C.Array":
    """The eight view words as the host array mmvae_plot_count_f32 reads."""
    words = [float(w) for w in view]
    if len(words) != 8:
        raise ValueError(f"a view is eight numbers (a00 a01 a02 b0 a10 a11 a12 b1), got {len(words)}")
    return (C.c_float * 8)(*words)
