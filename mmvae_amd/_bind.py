"""The one ctypes loader of the project's native libraries, and the two helpers every call site needs.

A library is described once, by a `Binding` next to its prototype table (`_lib`, the `_X_lib` satellites, `data` for the
host-side feed helper); `Binding.load()` opens it, binds every prototype and refuses a build whose ABI version is not the
one the table was written against.  The libraries are the product: missing or stale, every call raises -- there is no
fallback to torch ops ("no CPU fallback").
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_PACKAGE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_PACKAGE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_PACKAGE), "include")

# the modules that hold a device library's BINDING (a new library: one prototypes module, one Makefile line, one entry
# here); __graft_entry__.build() loads each and checks its version and build arch
DEVICE_LIBRARY_MODULES = ("_lib", "_stats_lib", "_disc_lib", "_umap_lib", "_hist_lib", "_prep_lib", "_plot_lib",
                          "_ckpt_lib", "_mix_lib", "_sil_lib")
# the libraries added since: a tuple of their own, because the suite pins the length of the one above
MORE_DEVICE_LIBRARY_MODULES = ("_clust_lib", "_graph_lib", "_pca_lib")


class HipLibraryError(RuntimeError):
    pass


class Binding:
    """One native library: its file, its header, its `name -> (restype, argtypes)` table and the ABI version that table
    was written against.  `arch_symbol` names the export that returns the build's GPU arch (None: host code)."""

    def __init__(self, so_name: str, header: str, prototypes: dict, version_symbol: str, abi_version: int,
                 arch_symbol: Optional[str] = None, needs_torch: bool = True):
        self.path = os.path.join(CSRC, so_name)
        self.header_path = os.path.join(INCLUDE, header)
        self.prototypes = prototypes
        self.version_symbol = version_symbol
        self.abi_version = abi_version
        self.arch_symbol = arch_symbol
        self.needs_torch = needs_torch
        self._lib: Optional[C.CDLL] = None

    def load(self) -> C.CDLL:
        """Open the library (built by __graft_entry__.build() / `make -C mmvae_amd/csrc`).  Raises loudly."""
        if self._lib is not None:
            return self._lib
        if self.needs_torch:
            # A device library works on torch's streams and device memory, so it must share torch's HIP runtime: torch
            # ships its own libamdhip64, and whichever copy is loaded first serves the whole process.  Loading the
            # library before torch binds its code objects to the system runtime, and every launch on a torch stream
            # then fails (MMVAE_ERR_LAUNCH).
            import torch  # noqa: F401

        path = self.path
        if not os.path.exists(path):
            raise HipLibraryError(
                f"{path} not found: build it with `make -C mmvae_amd/csrc` (or __graft_entry__.build()). "
                "mmvae_amd has no non-HIP execution path for device tensors."
            )
        try:
            lib = C.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise HipLibraryError(f"could not load {path}: {e}") from e
        for name, (res, args) in self.prototypes.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise HipLibraryError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        version = getattr(lib, self.version_symbol)()
        if version != self.abi_version:
            raise HipLibraryError(f"{path} has ABI {version}, this binding was written against {self.abi_version}: "
                                  "rebuild it")
        self._lib = lib
        return lib


def ptr(t) -> Optional[int]:
    """Address of a tensor's storage for a c_void_p argument (None stays None: an absent operand)."""
    return None if t is None else t.data_ptr()


def stream(device=None) -> int:
    """Handle of torch's current stream on `device` (None: the current device) for a hipStream_t argument."""
    import torch

    return torch.cuda.current_stream(device).cuda_stream
