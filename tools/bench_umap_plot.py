#!/usr/bin/env python3
"""Times the category rasteriser (libmmvae_plot.so) on a seeded Gaussian-mixture embedding with 15 classes, picture
1085 x 616, marker 1 pixel, at N = 1 000 000 and 3 000 000 points -- the figures of profiles/umap_plot.txt.

    python tools/bench_umap_plot.py                  # on the GPU: HIP against torch-on-device, the A/B, the host leg
    python tools/bench_umap_plot.py --resources      # no GPU: registers, LDS and spills of the kernels (hipcc -S)

Every device time is the median of --repeats (>= 20) runs behind --warmup runs, each between two device events and
ended by a synchronise, all in one process; the two ways of adding (plain atomics, wave aggregation) and the torch
formulation alternate inside the same loop.  The torch formulation is the same picture: the same float32 index
arithmetic, torch.bincount(minlength = C H W) and a torch composite; its counts must equal the kernel's.  The host leg
is the reference's plot_category written out afresh (pandas frame, shuffle, colour column, plt.scatter(s=1, alpha=0.5),
savefig) timed once at 200 000 points; its figure for the larger sizes is a LINEAR EXTRAPOLATION and is labelled so.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, C = 1085, 616, 15
HBM_BYTES_PER_S = 8.0e12


def resources() -> int:
    """Registers, LDS, scratch and spills of every kernel of plot_raster.hip, from the code object's metadata."""
    src = os.path.join(ROOT, "mmvae_amd", "csrc", "plot_raster.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "plot_raster.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-S", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    fields = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
              "sgpr_spill_count")
    print(f"{'kernel':58s} " + " ".join(f"{f.replace('_fixed_size', '').replace('_count', ''):>16s}" for f in fields))
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"plot_count_kernelILi(\d)ELb(\d)ELb(\d)", name)
        short = (f"plot_count_kernel<dims {m.group(1)}, {'packed' if m.group(2) == '1' else 'strided'}, "
                 f"{'aggregate' if m.group(3) == '1' else 'plain'}>") if m else "plot_composite_kernel"
        values = [re.search(r"\." + f + r":\s+(\d+)", block).group(1) for f in fields]
        print(f"{short:58s} " + " ".join(f"{v:>16s}" for v in values))
    return 0


def mixture(n, torch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.rand((C, 2), generator=g, device="cuda") * 16.0 - 8.0
    codes = torch.randint(0, C, (n,), generator=g, device="cuda", dtype=torch.int32)
    pts = centres[codes.long()] + 0.35 * torch.randn((n, 2), generator=g, device="cuda")
    return pts.contiguous(), codes


def torch_counts(pts, codes, view, torch):
    """The same index arithmetic as the kernel (separate float32 products and sums), then torch.bincount."""
    a = [torch.tensor(w, dtype=torch.float32, device="cuda") for w in view]
    x, y = pts[:, 0], pts[:, 1]
    u = (a[0] * x + a[1] * y) + a[3]
    v = (a[4] * x + a[5] * y) + a[7]
    fu, fv = torch.floor(u), torch.floor(v)
    keep = ((codes >= 0) & (codes < C) & torch.isfinite(u) & torch.isfinite(v) & (fu >= 0) & (fu <= W - 1) & (fv >= 0)
            & (fv <= H - 1))
    lin = (codes.long() * H + fv.long()) * W + fu.long()
    return torch.bincount(lin[keep], minlength=C * H * W).view(C, H, W)


def torch_composite(counts, colors, alpha, torch):
    nc = counts.to(torch.float32)
    n = nc.sum(0)
    mean = torch.einsum("chw,ck->hwk", nc, colors) / n.clamp_min(1.0)[..., None]
    t = torch.pow(torch.tensor(1.0 - alpha, device="cuda"), n)[..., None]
    rgb = torch.where(n[..., None] > 0, (1.0 - t) * mean + t, torch.ones_like(mean))
    out = torch.full((H, W, 4), 255, dtype=torch.uint8, device="cuda")
    out[..., :3] = torch.round(255.0 * rgb).clamp(0, 255).to(torch.uint8)
    return out


def host_scatter_seconds(n: int) -> float:
    """The reference's plot_category, written out afresh, on n points: seconds of host time for one image."""
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    import pandas as pd

    rng = np.random.default_rng(0)
    centres = rng.uniform(-8, 8, (C, 2))
    labels = rng.integers(0, C, n)
    emb = centres[labels] + 0.35 * rng.standard_normal((n, 2))
    metadata = pd.DataFrame({"cell_type": [f"type{i}" for i in labels]})
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        plt.figure(figsize=(14, 8))
        top = metadata["cell_type"].value_counts().nlargest(15).index
        cmap = plt.get_cmap("nipy_spectral", len(top))
        color_of = {value: cmap(i) for i, value in enumerate(top)}
        df = pd.DataFrame(emb, columns=["x", "y"])
        df["cell_type"] = metadata["cell_type"].values
        df = df[df["cell_type"].isin(top)].sample(frac=1).reset_index(drop=True)
        df["color"] = df["cell_type"].map(color_of)
        plt.scatter(x=df["x"], y=df["y"], c=df["color"], s=1, alpha=0.5)
        plt.title("UMAP projection colored by cell_type")
        plt.savefig(os.path.join(tmp, "host.png"), bbox_inches="tight")
        plt.close()
        return time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=200_000)
    ap.add_argument("--no-host", action="store_true", help="skip the plt.scatter leg")
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers, LDS and spills; no GPU")
    args = ap.parse_args()
    if args.resources:
        return resources()
    if args.repeats < 20:
        ap.error("--repeats: at least 20")
    import torch

    if not torch.cuda.is_available():
        print("bench_umap_plot: no GPU -- nothing is measured without one", file=sys.stderr)
        return 2
    from mmvae_amd import _plot_lib, plots

    lib = _plot_lib.load_plot()
    stream = torch.cuda.current_stream().cuda_stream
    colors = torch.rand((C, 3), generator=torch.Generator().manual_seed(1)).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}; picture {W} x {H}, {C} classes, marker 1 px, alpha 0.5; "
          f"median of {args.repeats} behind {args.warmup} warm-up runs, device events")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)  # ms

    host = None
    if not args.no_host:
        try:
            host_scatter_seconds(2000)  # (imports and font caches)
            host = host_scatter_seconds(args.host_points)
            print(f"host plt.scatter path, {args.host_points} points: {host:.2f} s per image (measured, this host's CPU)")
        except ImportError as e:
            print(f"host plt.scatter path: skipped, matplotlib is not installed ({e})")

    for n in args.sizes:
        pts, codes = mixture(n, torch)
        view = plots.fit_view(pts, codes, W, H)
        words = _plot_lib.view_words(view)
        counts = torch.empty((C, H, W), dtype=torch.int32, device="cuda")
        rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")

        def count(mode):
            _plot_lib.check(lib.mmvae_plot_count_f32(n, 2, pts.data_ptr(), 2, codes.data_ptr(), C, W, H, 1, words, mode,
                                                     counts.data_ptr(), stream), "count")

        def composite():
            _plot_lib.check(lib.mmvae_plot_composite_u8(counts.data_ptr(), C, W, H, colors.data_ptr(), 0.5, 1.0, 1.0, 1.0,
                                                        rgba.data_ptr(), stream), "composite")

        def both():
            count(_plot_lib.PLOT_COUNT_DEFAULT)
            composite()

        kept = {}

        def torch_count():
            kept["counts"] = torch_counts(pts, codes, view, torch)

        def torch_comp():
            kept["rgba"] = torch_composite(kept["counts"], colors, 0.5, torch)

        def torch_both():
            torch_count()
            torch_comp()

        legs = {"hip count, plain atomics": lambda: count(_plot_lib.PLOT_COUNT_PLAIN),
                "hip count, wave aggregation": lambda: count(_plot_lib.PLOT_COUNT_AGGREGATE),
                "hip count (default mode)": lambda: count(_plot_lib.PLOT_COUNT_DEFAULT),
                "hip composite": composite, "hip count + composite": both,
                "torch count (bincount)": torch_count, "torch composite": torch_comp, "torch count + composite": torch_both}
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, fn in legs.items():  # the legs alternate inside one loop
                ms = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        # the same picture?
        both()
        torch_both()
        torch.cuda.synchronize()
        same_counts = bool(torch.equal(counts.long(), kept["counts"]))
        diff = (rgba.int() - kept["rgba"].int()).abs()
        on_top = int(counts.view(C, -1).sum(0).max())
        print(f"\nN = {n}: {int(counts.sum())} points counted, the fullest pixel holds {on_top}; counts equal torch's: "
              f"{same_counts}; composite differs from torch's by at most {int(diff.max())} "
              f"({100 * float((diff > 0).float().mean()):.3f} % of bytes)")
        for k in legs:
            v = times[k]
            print(f"  {k:30s} {med[k] * 1e3:10.1f} us   (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")
        hip, tor = med["hip count + composite"], med["torch count + composite"]
        print(f"  torch / hip, count + composite: {tor / hip:.2f} x   ({'HIP is not slower' if hip <= tor else 'HIP IS SLOWER'})")
        print(f"  aggregation / plain: {med['hip count, wave aggregation'] / med['hip count, plain atomics']:.2f} x")
        rate = 12.0 * n / (med["hip count (default mode)"] * 1e-3)
        print(f"  count kernel: 12 B per point read once = {12.0 * n / 1e6:.1f} MB in {med['hip count (default mode)'] * 1e3:.1f} us "
              f"(the clearing memset of {4 * C * H * W / 1e6:.1f} MB included) = {rate / 1e12:.3f} TB/s, "
              f"{100 * rate / HBM_BYTES_PER_S:.1f} % of 8 TB/s")
        crate = (4.0 * C + 4.0) * H * W / (med["hip composite"] * 1e-3)
        print(f"  composite kernel: {(4.0 * C + 4.0) * H * W / 1e6:.1f} MB read and written = {crate / 1e12:.3f} TB/s, "
              f"{100 * crate / HBM_BYTES_PER_S:.1f} % of 8 TB/s")
        if host is not None:
            est = host * n / args.host_points
            print(f"  host plt.scatter path at this N: {est:.1f} s per image -- a LINEAR EXTRAPOLATION from "
                  f"{args.host_points} points, not measured; against it the HIP path is {est / (hip * 1e-3):.0f} x")
        if not same_counts or int(diff.max()) > 1:
            print("bench_umap_plot: the two formulations disagree", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
