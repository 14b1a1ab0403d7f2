#!/usr/bin/env python3
"""The integration metrics on the latent kNN graph (libmmvae_mix.so, mmvae_amd.mixing), measured.

    python tools/bench_mixing.py                  # on the GPU; the lines also go to --out (default profiles/mixing.txt)
    python tools/bench_mixing.py --resources      # no GPU: registers, LDS, scratch, spills and occupancy of the kernels

Data: a seeded mixture of 15 Gaussian clusters in 128 dimensions, two batches, the cluster as the label, at N = 100 000
and 1 000 000 cells, k = 64, perplexity 21.  One child process per size, each under its own time limit (a size that
faults, aborts or runs out of time ends the run: nothing more is started on the device).  Per size:

  entries    ms of mmvae_mix_calibrate_f32, mmvae_mix_lisi_f32 (two columns, one launch) and mmvae_mix_transfer_f32 on
             the graph of umap.knn_graph, device events around blocks of calls, three blocks interleaved with
  torch      the same definition written with vectorised torch ops on the same device (mixing._calibrate_torch,
             _lisi_torch, _transfer_torch: the module's fp64 statement, one masked step per try and one per rank), and
             how far the two agree
  whole      s of mixing.integration_metrics(z, metadata), host clock around a synchronised call, and of its stages
  host       the numpy row loop (one row at a time, the way the published implementation walks its cells) on the
             first --host-rows rows, on this host's CPU; its figure for the whole N is a LINEAR EXTRAPOLATION and is
             labelled so

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

SIZES = [100_000, 1_000_000]
K, D, CLUSTERS, PERPLEXITY = 64, 128, 15, 21.0
LIMIT = {100_000: 300, 1_000_000: 600}  # seconds per child


def resources() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
              "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_mix.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / SGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(ROOT, "mmvae_amd", "csrc", "knn_mix.hip"), "-o", os.path.join(tmp, "dev.o")],
                             capture_output=True, text=True, check=True).stderr
    name, row = None, {}
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
            print(f"  {demangled.split('::')[-1]:24s} " + " / ".join(row[f] for f in fields))
            name = None
    return 0


def mixture(n, torch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = 2.0 * torch.randn(CLUSTERS, D, device="cuda", generator=g)
    cluster = torch.randint(0, CLUSTERS, (n,), device="cuda", generator=g)
    batch = torch.randint(0, 2, (n,), device="cuda", generator=g)
    z = centres[cluster] + torch.randn(n, D, device="cuda", generator=g)
    return z, batch.to(torch.int32), cluster.to(torch.int32)


# ------------------------------------------------------------------------------------- the numpy row loop on the host
def host_row(np, d32, codes_nb, batch_i, batch_nb, label_nb):
    """One cell: calibration, LISI of every code column and the transfer, numpy on one row."""
    d = d32[1:].astype(np.float64) - float(d32[1])
    log_u = math.log(PERPLEXITY)
    beta, lo, hi, tries = 1.0, -math.inf, math.inf, 0
    while True:
        e = np.exp(-beta * d)
        s = e.sum()
        p = e / s
        h = math.log(s) + beta * float((d * p).sum())
        if not (abs(h - log_u) > 1e-5 and tries < 50):
            break
        if h > log_u:
            lo, beta = beta, (beta * 2.0 if hi == math.inf else (beta + hi) / 2.0)
        else:
            hi, beta = beta, (beta / 2.0 if lo == -math.inf else (beta + lo) / 2.0)
        tries += 1
    out = []
    for c in codes_nb:
        keep = c >= 0
        _, inv = np.unique(c[keep], return_inverse=True)
        mass = np.bincount(inv, weights=p[keep])
        out.append(p[keep].sum() ** 2 / (mass * mass).sum() if keep.any() else math.nan)
    ok = (batch_nb >= 0) & (batch_nb != batch_i) & (label_nb >= 0)
    if ok.any():
        labels, inv = np.unique(label_nb[ok], return_inverse=True)
        mass = np.bincount(inv, weights=p[ok])
        out += [labels[mass.argmax()], mass.max() / mass.sum(), mass.sum()]
    else:
        out += [-1, 0.0, 0.0]
    return beta, out


def host_seconds(idx, dist, batch, label, rows):
    import numpy as np

    idx, dist, batch, label = (t.cpu().numpy() for t in (idx[:rows], dist[:rows], batch, label))
    t0 = time.perf_counter()
    for i in range(rows):
        nb = idx[i, 1:]
        host_row(np, dist[i], (batch[nb], label[nb]), batch[i], batch[nb], label[nb])
    return time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------------- one size
def child(n: int, host_rows: int) -> int:
    import pandas as pd
    import torch

    if not torch.cuda.is_available():
        print("bench_mixing: no GPU -- nothing is measured without one", file=sys.stderr)
        return 2
    from mmvae_amd import mixing
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
    idx, dist = U.knn_graph(z, K)
    codes = torch.stack([batch, label])
    beta, tries = mixing.calibrate(idx, dist, PERPLEXITY)
    legs = {
        "calibrate": (lambda: mixing.calibrate(idx, dist, PERPLEXITY),
                      lambda: mixing._calibrate_torch(dist, PERPLEXITY)),
        "lisi, 2 columns": (lambda: mixing.lisi(idx, dist, codes, beta=beta, _trusted=True),
                            lambda: mixing._lisi_torch(idx, dist, beta, codes)),
        "transfer": (lambda: mixing.label_transfer(idx, dist, batch, label, beta=beta, _trusted=True),
                     lambda: mixing._transfer_torch(idx, dist, beta, batch, label)),
    }
    reps_hip, reps_torch = (20, 3) if n <= 200_000 else (5, 1)
    print(f"\nN = {n}, k = {K}, D = {D}, {CLUSTERS} clusters, 2 batches, perplexity {PERPLEXITY:g} on "
          f"{torch.cuda.get_device_name(0)}; tries: median {int(tries.double().median())}, max {int(tries.max())}")
    print(f"  3 interleaved blocks of {reps_hip} (HIP) and {reps_torch} (torch) calls, device events, after a warm-up "
          "call of each; ms per call, the median block")
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    total_hip = total_torch = 0.0
    for name, (hip, stock) in legs.items():
        hip()
        stock()
        torch.cuda.synchronize()
        t_hip, t_stock = [], []
        for _ in range(3):
            t_hip.append(events(hip, reps_hip))
            t_stock.append(events(stock, reps_torch))
        total_hip, total_torch = total_hip + med(t_hip), total_torch + med(t_stock)
        verdict = "HIP is not slower" if med(t_hip) <= med(t_stock) else "HIP IS SLOWER"
        print(f"  {name:16s} HIP {med(t_hip):10.3f} ms (blocks {' '.join(f'{v:.3f}' for v in t_hip)})   torch "
              f"{med(t_stock):10.3f} ms (blocks {' '.join(f'{v:.3f}' for v in t_stock)})   torch / HIP "
              f"{med(t_stock) / med(t_hip):8.2f} x   {verdict}")
    print(f"  the three entries  HIP {total_hip:10.3f} ms   torch {total_torch:10.3f} ms   torch / HIP "
          f"{total_torch / total_hip:8.2f} x")
    # the same numbers?
    tb, tt = mixing._calibrate_torch(dist, PERPLEXITY)
    tl = mixing._lisi_torch(idx, dist, beta, codes)
    tp, tc, tx = mixing._transfer_torch(idx, dist, beta, batch, label)
    hl = mixing.lisi(idx, dist, codes, beta=beta, _trusted=True).double()
    hp, hc, hx = mixing.label_transfer(idx, dist, batch, label, beta=beta, _trusted=True)
    rel = lambda a, b: float(((a - b).abs() / b.abs()).nan_to_num(0.0).max())  # noqa: E731
    print(f"  agreement with torch: beta bit-equal on {100 * float((tb == beta).double().mean()):.4f} % of the rows, tries "
          f"equal on {100 * float((tt == tries).double().mean()):.4f} %; lisi differs by at most {rel(hl, tl):.2e} relative, "
          f"cross by {rel(hx.double(), tx):.2e}; pred equal on {100 * float((hp == tp).double().mean()):.4f} %")
    del tb, tt, tl, tp, tc, tx, hl
    # the whole call
    names = [f"type{i:02d}" for i in range(CLUSTERS)]
    lab, bat = label.cpu().numpy(), batch.cpu().numpy()
    metadata = pd.DataFrame({"species": ["human" if b == 0 else "mouse" for b in bat], "cell_type": [names[c] for c in lab]})
    mixing.integration_metrics(z, metadata)
    whole = [clock(lambda: mixing.integration_metrics(z, metadata))[0] for _ in range(3)]
    t_knn, _ = clock(lambda: U.knn_graph(z, K))
    t_fac, _ = clock(lambda: [mixing.factorize(metadata[c]) for c in ("species", "cell_type")])
    out = mixing.integration_metrics(z, metadata)
    t_sum, _ = clock(lambda: (mixing.summarise_lisi(out.lisi, out.columns, ["batch", "label"], [2, CLUSTERS]),
                              mixing.summarise_transfer("cell_type", out.codes[0], out.codes[1], out.pred["cell_type"],
                                                        out.cross["cell_type"], ["human", "mouse"], names)))
    print(f"  integration_metrics(z, metadata): {sorted(whole)[1]:.3f} s (calls {' '.join(f'{v:.3f}' for v in whole)}); "
          f"of it kNN graph {t_knn:.3f} s, pandas.factorize of two columns on the host {t_fac:.3f} s, the three entries "
          f"{total_hip * 1e-3:.4f} s, the summary tables {t_sum:.3f} s")
    s = out.summary
    print(f"  result: median LISI species {s['median_lisi'][0]:.3f} of 2, cell_type {s['median_lisi'][1]:.3f} of {CLUSTERS}; "
          f"transfer accuracy {out.transfer_summary['accuracy'].tolist()[-1]:.4f}")
    rows = min(host_rows, n)
    host_seconds(idx, dist, batch, label, min(50, rows))
    t_host = host_seconds(idx, dist, batch, label, rows)
    est = t_host * n / rows
    print(f"  numpy row loop on this host's CPU, the same three results per cell: {t_host:.3f} s for {rows} rows "
          f"(measured); {est:.1f} s for all {n} rows -- a LINEAR EXTRAPOLATION, not measured; against it the three HIP "
          f"entries are {est / (total_hip * 1e-3):.0f} x")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--host-rows", type=int, default=2000, help="rows the numpy row loop is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixing.txt"))
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers, LDS and spills; no GPU")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.resources:
        return resources()
    if args.child:
        return child(args.child, args.host_rows)
    lines, rc = [], 0
    for n in args.sizes:
        limit = LIMIT.get(n, 600)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--host-rows",
                                str(args.host_rows)], capture_output=True, text=True, timeout=limit)
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
