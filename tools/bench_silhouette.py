#!/usr/bin/env python3
"""The silhouette widths of latent embeddings (libmmvae_sil.so, mmvae_amd.silhouette), measured.

    python tools/bench_silhouette.py                  # on the GPU; the lines also go to --out (default profiles/silhouette.txt)
    python tools/bench_silhouette.py --resources      # no GPU: registers, LDS, scratch, spills and occupancy of the kernels
    rocprofv3 --kernel-trace --stats -- python tools/bench_silhouette.py --once 100000   # kernel times, a run of its own

Data: a seeded mixture of 15 Gaussian clusters in 128 dimensions, two batches, the cluster as the label, at N = 20 000 and
100 000 cells, both metrics.  One child process per size, each under its own time limit (a size that faults, aborts or
runs out of time ends the run: nothing more is started on the device).  Per size and metric:

  label      ms of mmvae_sil_rows_f32 with class = label over one group (R = 15: N^2 pairs)
  batch      ms of mmvae_sil_rows_f32 with class = batch, group = label (R = 30, 15 groups: sum_g n_g^2 pairs)
  torch      the same definition with torch ops on the same device: cdist (or a matmul of unit rows) on chunks of rows and
             a one-hot matmul per chunk, and how far the two agree
  kNN        ms of mmvae_umap_knn_cosine_f32 at the same (N, D), k = 30: the yardstick for the same Gram work
  whole      s of silhouette.silhouette_widths(z, metadata), host clock around a synchronised call

All four are timed in one process, alternating, after a warm-up call of each; device events around blocks of calls that
last at least 0.5 s.  TFLOP/s are the algorithmic 2 pairs D over the ENTRY's time (its row and norm passes included; the
kernel-only figures come from the rocprofv3 run above and stand at the end of profiles/silhouette.txt and in DESIGN §6i;
a plain run rewrites the file without them), beside their share of the 157.3 TFLOP/s fp32-MFMA peak.
scikit-learn's silhouette_samples runs on this host's CPU at --host-rows cells where it is importable; its figure for the
whole N is a QUADRATIC EXTRAPOLATION and is labelled "not measured".

Nothing is asserted: the numbers are reported.
"""
import argparse
import math
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [20_000, 100_000]
D, CLUSTERS, K = 128, 15, 30
PEAK = 157.3e12
LIMIT = {20_000: 240, 100_000: 420}  # seconds per child


def resources() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
              "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_sil.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / SGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(ROOT, "mmvae_amd", "csrc", "sil_rows.hip"), "-o", os.path.join(tmp, "dev.o")],
                             capture_output=True, text=True, check=True).stderr
    name, row, spills = None, {}, 0
    for line in out.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name, row = m.group(1), {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
        if m and name:
            row[m.group(1).strip()] = m.group(2)
        if name and all(f in row for f in fields):
            demangled = subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip() or name
            print(f"  {demangled.split('::')[-1]:32s} " + " / ".join(row[f] for f in fields))
            spills += int(row["VGPRs Spill"]) + int(row["SGPRs Spill"]) + int(row["ScratchSize [bytes/lane]"])
            name = None
    print("no kernel spills" if spills == 0 else "SOME KERNEL SPILLS")
    return 0


def mixture(n, torch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = 2.0 * torch.randn(CLUSTERS, D, device="cuda", generator=g)
    cluster = torch.randint(0, CLUSTERS, (n,), device="cuda", generator=g)
    batch = torch.randint(0, 2, (n,), device="cuda", generator=g)
    z = centres[cluster] + torch.randn(n, D, device="cuda", generator=g)
    return z, batch.to(torch.int32), cluster.to(torch.int32)


def torch_rows(torch, x, metric, run_ptr, run_group, chunk=4096):
    """(a, b) fp32 of sorted rows by the definition in stock torch ops: per chunk of rows the distances to all rows and
    their sums per run through a one-hot matmul."""
    n, R = x.shape[0], run_group.numel()
    counts = (run_ptr[1:] - run_ptr[:-1]).long()
    run_of = torch.repeat_interleave(torch.arange(R, device=x.device), counts)
    onehot = torch.zeros((n, R), dtype=torch.float32, device=x.device)
    onehot[torch.arange(n, device=x.device), run_of] = 1.0
    if metric == "cosine":
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    sums = torch.empty((n, R), dtype=torch.float32, device=x.device)
    for i0 in range(0, n, chunk):
        rows = x[i0:i0 + chunk]
        d = (1.0 - rows @ x.T).clamp_min(0.0) if metric == "cosine" else torch.cdist(rows, x)
        sums[i0:i0 + chunk] = d @ onehot
    cnt = counts.float()
    own = onehot.bool()
    n_own = cnt[run_of]
    a = sums[own] / (n_own - 1).clamp_min(1.0)
    other = (run_group[run_of][:, None] == run_group[None, :]) & ~own
    b = torch.where(other, sums / cnt[None, :], torch.full_like(sums, float("inf"))).min(1).values
    return a, b


def child(n: int, host_rows: int, once: bool) -> int:
    import pandas as pd
    import torch

    if not torch.cuda.is_available():
        print("bench_silhouette: no GPU -- nothing is measured without one", file=sys.stderr)
        return 2
    from mmvae_amd import silhouette as S
    from mmvae_amd import umap as U

    def events(fn, reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / reps

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    z, batch, label = mixture(n, torch)
    z64 = z.double()
    centred = (z64 - z64.mean(0, keepdim=True)).float()
    del z64
    o1, p1, g1, _ = S.sort_runs(label)
    o2, p2, g2, _ = S.sort_runs(batch, label)
    pairs = {"label": float(n) * n, "batch": float(((p1[1:] - p1[:-1]).double() ** 2).sum())}
    print(f"\nN = {n}, D = {D}, {CLUSTERS} clusters, 2 batches on {torch.cuda.get_device_name(0)}; pairs: label "
          f"{pairs['label']:.3e}, batch {pairs['batch']:.3e}")
    if once:  # one call of each entry, for a kernel trace
        for metric in ("euclidean", "cosine"):
            rows = centred if metric == "euclidean" else z
            S.silhouette_rows(rows[o1], p1, g1, metric)
            S.silhouette_rows(rows[o2], p2, g2, metric)
        U.knn_graph(z, K)
        torch.cuda.synchronize()
        print("  one call of each entry made")
        return 0
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for metric in ("euclidean", "cosine"):
        rows = centred if metric == "euclidean" else z
        x1, x2 = rows[o1].contiguous(), rows[o2].contiguous()
        legs = {"label": lambda: S.silhouette_rows(x1, p1, g1, metric),
                "batch": lambda: S.silhouette_rows(x2, p2, g2, metric),
                "torch label": lambda: torch_rows(torch, x1, metric, p1, g1),
                "kNN k=30": lambda: U.knn_graph(z, K)}
        reps = {}
        for name, fn in legs.items():  # warm-up, and the calls that fill 0.5 s
            fn()
            reps[name] = max(1, int(math.ceil(0.5 / max(clock(fn)[0], 1e-4))))
        times = {name: [] for name in legs}
        for _ in range(3):
            for name, fn in legs.items():
                times[name].append(events(fn, reps[name]))
        print(f"  {metric}: 3 alternating blocks of >= 0.5 s, device events, ms per call, the median block")
        for name in legs:
            t = med(times[name])
            line = f"    {name:12s} {t:10.3f} ms (blocks {' '.join(f'{v:.3f}' for v in times[name])}; {reps[name]} calls each)"
            if name in pairs:
                flops = 2.0 * pairs[name] * D / (t * 1e-3)
                line += f"   {flops / 1e12:6.1f} TFLOP/s of the entry = {100 * flops / PEAK:4.1f} % of the fp32-MFMA peak"
            if name == "kNN k=30":
                flops = 2.0 * float(n) * n * D / (t * 1e-3)
                line += f"   {flops / 1e12:6.1f} TFLOP/s (umap.knn_graph: the entry and its workspace allocation)"
            print(line)
        t_label, t_knn, t_torch = med(times["label"]), med(times["kNN k=30"]), med(times["torch label"])
        print(f"    label entry / kNN entry {t_label / t_knn:.2f} x ({'the silhouette pass is the slower' if t_label > t_knn else 'the silhouette pass is not slower'}); "
              f"torch / label entry {t_torch / t_label:.2f} x ({'HIP is not slower' if t_label <= t_torch else 'HIP IS SLOWER'})")
        a, b, s, _ = S.silhouette_rows(x1, p1, g1, metric)
        ta, tb = torch_rows(torch, x1, metric, p1, g1)
        print(f"    agreement with torch (fp32 throughout): a differs by at most {float((a - ta).abs().max()):.2e}, b by "
              f"{float((b - tb).abs().max()):.2e} at a largest mean distance of {float(torch.maximum(a, b).max()):.3f}")
        del a, b, s, ta, tb, x1, x2
    names = [f"type{i:02d}" for i in range(CLUSTERS)]
    lab, bat = label.cpu().numpy(), batch.cpu().numpy()
    metadata = pd.DataFrame({"species": ["human" if v == 0 else "mouse" for v in bat], "cell_type": [names[c] for c in lab]})
    S.silhouette_widths(z, metadata)
    whole = [clock(lambda: S.silhouette_widths(z, metadata))[0] for _ in range(3)]
    out = S.silhouette_widths(z, metadata)
    print(f"  silhouette_widths(z, metadata), euclidean: {sorted(whole)[1]:.3f} s (calls {' '.join(f'{v:.3f}' for v in whole)}); "
          f"result: label ASW {out.summary['asw'][0]:.4f} (scaled {out.summary['scaled'][0]:.4f}), batch ASW "
          f"{out.summary['asw'][1]:.4f}")
    try:
        from sklearn.metrics import silhouette_samples
    except ImportError:
        print("  scikit-learn is not importable here: the host figure is not measured")
        return 0
    rows = min(host_rows, n)
    xs, ls = z[:rows].cpu().numpy(), lab[:rows]
    t0 = time.perf_counter()
    silhouette_samples(xs, ls)
    t_host = time.perf_counter() - t0
    print(f"  sklearn.metrics.silhouette_samples on this host's CPU: {t_host:.3f} s for {rows} cells (measured); "
          f"{t_host * (n / rows) ** 2:.1f} s for all {n} cells -- a QUADRATIC EXTRAPOLATION, not measured")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--host-rows", type=int, default=5000, help="cells scikit-learn is timed on (at most 10 000)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette.txt"))
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers, LDS and spills; no GPU")
    ap.add_argument("--once", type=int, help="one call of each entry at this N, in this process (for a kernel trace)")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    host_rows = min(args.host_rows, 10_000)
    if args.resources:
        return resources()
    if args.once:
        return child(args.once, host_rows, True)
    if args.child:
        return child(args.child, host_rows, False)
    lines, rc = [], 0
    for n in args.sizes:
        limit = LIMIT.get(n, 420)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--host-rows",
                                str(host_rows)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"[N = {n}] ran past its {limit} s limit: stopping here")
            print(lines[-1])
            rc = 1
            break
        sys.stdout.write(p.stdout)
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"[N = {n}] exited with {p.returncode}: stopping here\n{p.stderr[-2000:]}")
            print(lines[-1])
            rc = 1
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
