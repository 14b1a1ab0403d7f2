"""ctypes binding of libmmvae_graph.so (the C-ABI declared in include/mmvae_graph.h): connected components of a neighbour
table, the component sizes per class, and the kBET chi-square test of every neighbourhood's batch composition.

A satellite device library with its own version counter, so that it moves neither the training step's ABI nor another
satellite's.  Like `_lib`, it is the product: missing or unloadable, every call raises -- no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ._bind import Binding
from ._lib import ERR_ARG, ERR_LAUNCH, OK, HipLibraryError, check  # noqa: F401  (the return codes are shared)

GRAPH_ABI_VERSION = 1
GRAPH_MAX_K = 64
GRAPH_MAX_BATCHES = 64

_p = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes), in the order of include/mmvae_graph.h (tests/test_graph_metrics_host.py checks that every
# symbol the header declares is listed here and exported by the .so)
GRAPH_PROTOTYPES = {
    "mmvae_graph_abi_version": (_i, []),
    "mmvae_graph_build_arch": (C.c_char_p, []),
    "mmvae_graph_cc_round_i32": (_i, [_i, _i, _p, _p, _p, _p, _p]),
    "mmvae_graph_component_sizes_i32": (_i, [_i, _p, _p, _i, _p, _p, _p, _p, _p]),
    "mmvae_graph_kbet_f64": (_i, [_i, _i, _p, _p, _i, _p, _i, _p, _p, _p]),
}

BINDING = Binding("libmmvae_graph.so", "mmvae_graph.h", GRAPH_PROTOTYPES, "mmvae_graph_abi_version", GRAPH_ABI_VERSION,
                  "mmvae_graph_build_arch")
GRAPH_LIB_PATH = BINDING.path

_graph: Optional[C.CDLL] = None


def load_graph() -> C.CDLL:
    """Load libmmvae_graph.so (see _bind.Binding.load).  Raises loudly."""
    global _graph
    if _graph is not None:
        return _graph
    _graph = BINDING.load()
    return _graph
