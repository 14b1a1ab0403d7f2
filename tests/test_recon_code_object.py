"""Host-only check of the built library's code object: the wave-specialised reconstruction kernels (the fused last
decoder layer, gemm_x3w_kernel<..., EPI_RECON, ...>) must not use scratch memory.  Their epilogue runs from LDS on all
eight waves precisely so that nothing of it is spilled; a spill that comes back shows up here, without a GPU, as a
non-zero .private_segment_fixed_size in the kernel's metadata note.  Only metadata is read, no instructions."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mmvae_amd", "csrc", "libmmvae_hip.so")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _readelf():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.path.join(rocm, "llvm", "bin", "llvm-readelf"), os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf")):
        if os.path.isfile(cand):
            return cand
    return shutil.which("llvm-readelf")


def _gfx950_code_objects(blob):
    """The device ELF images of every (uncompressed) offload bundle in the library: one bundle per translation unit."""
    pos = 0
    while True:
        i = blob.find(BUNDLE_MAGIC, pos)
        if i < 0:
            return
        pos = i + len(BUNDLE_MAGIC)
        (count,) = struct.unpack_from("<Q", blob, pos)
        if count > 64:  # the magic as a plain string somewhere else
            continue
        o = pos + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, o)
            triple = blob[o + 24:o + 24 + tlen]
            o += 24 + tlen
            if b"gfx950" in triple and size and blob[i + off:i + off + 4] == b"\x7fELF":
                yield blob[i + off:i + off + size]


def _private_sizes(readelf, elf_path):
    """[(kernel name, .private_segment_fixed_size)]: the metadata is a YAML list of per-kernel maps with sorted keys, so
    within one map .name comes before .private_segment_fixed_size."""
    out = subprocess.run([readelf, "--notes", elf_path], check=True, capture_output=True, text=True).stdout
    res, name = [], None
    for line in out.splitlines():
        if re.match(r"\s*- \.", line):  # a new list item: a new kernel (or a new argument) map begins
            name = None if ".name:" not in line else re.search(r"\.name:\s+(\S+)", line).group(1)
        m = re.search(r"^\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", line)
        if m:
            assert name, "a private segment size without a kernel name before it"
            res.append((name, int(m.group(1))))
            name = None
    return res


def test_wave_specialised_recon_kernels_use_no_scratch(tmp_path):
    readelf = _readelf()
    if not os.path.isfile(LIB) or not readelf:
        pytest.skip("needs the built libmmvae_hip.so and the ROCm llvm-readelf")
    with open(LIB, "rb") as f:
        blob = f.read()
    seen = {}
    for k, elf in enumerate(_gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(elf)
        for name, private in _private_sizes(readelf, str(path)):
            # gemm_x3w_kernel<AFORM, BFORM, BM, BN, WGM, WGN, EPI, ASRC, BSRC>, mangled: ...ILi0ELi0ELi256ELi160ELi4ELi1ELi1E...
            m = re.search(r"gemm_x3w_kernelI((?:Li\d+E)+)E", name)
            if not m:
                continue
            args = [int(v) for v in re.findall(r"Li(\d+)E", m.group(1))]
            assert len(args) == 9, name
            if args[6] == 1:  # EPI_RECON
                seen[tuple(args)] = private
    # both tiles the planner can choose, over fp32 operands and over the two planes-operand forms
    for tile in ((256, 160, 4, 1), (256, 128, 2, 2)):
        for src in ((0, 0), (1, 0), (1, 1)):
            assert (0, 0) + tile + (1,) + src in seen, (tile, src, sorted(seen))
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
