"""The C-ABI surface check every native library gets (no GPU: nothing is launched).  A helper module, used by the host
test of each library with that library's `mmvae_amd._bind.Binding`."""
import re


def declared(header_text: str) -> dict:
    """name -> argument count of every mmvae_* function the header declares."""
    code = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    out = {}
    for m in re.finditer(r"\b(mmvae_\w+)\s*\(([^;{]*?)\)\s*;", code, re.S):
        args = [a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        out[m.group(1)] = len(args)
    return out


def check_surface(binding, version_define: bool = True) -> dict:
    """The header, the prototype table and the built library of `binding` describe the same surface: the same names,
    the same argument counts, one version number (the header's #define too, unless the header has none:
    `version_define=False`), a gfx950 build where the library reports an arch, and no exported mmvae_* symbol that the
    header does not declare.  Returns declared(header) for the caller's own pinned expectations."""
    header = open(binding.header_path).read()
    names = declared(header)
    assert set(binding.prototypes) == set(names), sorted(set(binding.prototypes) ^ set(names))
    lib = binding.load()  # loads on a GPU-less host too (no compute call is made)
    for name, n_args in names.items():
        assert hasattr(lib, name), f"declared in the header but not exported: {name}"
        assert len(binding.prototypes[name][1]) == n_args, name
    version = getattr(lib, binding.version_symbol)()
    assert version == binding.abi_version
    if version_define:
        define = re.search(r"#define\s+" + binding.version_symbol.upper() + r"\s+(\d+)", header)
        assert int(define.group(1)) == version
    if binding.arch_symbol is not None:
        assert getattr(lib, binding.arch_symbol)() == b"gfx950"
    # a retired entry point is gone from the library too (candidates: every mmvae_* name in the file's string tables;
    # exported: the loader resolves it)
    image = open(binding.path, "rb").read()
    strings = {m.decode() for m in re.findall(rb"(?<![A-Za-z0-9_])mmvae_[a-z0-9_]+(?=\x00)", image)}
    assert set(names) <= strings, "the scan of the string tables misses exported names"
    stale = sorted(n for n in strings - set(names) if hasattr(lib, n))
    assert not stale, f"exported but not declared in the header: {stale}"
    return names
