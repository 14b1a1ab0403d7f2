#!/usr/bin/env python3
"""K-means on latent embeddings (libmmvae_clust.so, mmvae_amd.clustering), measured.

    python tools/bench_kmeans.py                  # on the GPU; the lines also go to --out (default profiles/kmeans.txt)
    python tools/bench_kmeans.py --resources      # no GPU: registers, LDS, scratch, spills and occupancy of the kernels
    rocprofv3 --kernel-trace --stats -- python tools/bench_kmeans.py --once 1000000   # kernel times, a run of its own

Data: a seeded mixture of C Gaussian clusters in 128 dimensions at N = 100 000 and 1 000 000 rows, C = 15 and 64.  One
child process per N, each under its own time limit (a size that faults, aborts or runs out of time ends the run: nothing
more is started on the device).  Per (N, C):

  step       ms of mmvae_clust_kmeans_step_f32 (one whole Lloyd iteration: four launches) on preallocated buffers, and the
             bytes of x it has to read once, 4 N D, over that time
  seed pass  ms of mmvae_clust_seed_update_f32 (one round of k-means++ without its draw)
  torch      the same iteration with torch ops on the same device: cdist on chunks of rows, argmin, index_add_, bincount;
             and how far the two agree
  fit        s of clustering.kmeans_fit(z, C), host clock around a synchronised call, with its iterations
  sklearn    KMeans(algorithm="lloyd", n_init=1) on this host's CPU on at most --host-rows rows, where importable

The device legs are timed in one process, alternating, after a warm-up call of each; device events around blocks of calls
that last at least 0.5 s.  Nothing is asserted: the numbers are reported.
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
D, CLUSTERS = 128, (15, 64)
LIMIT = {100_000: 300, 1_000_000: 540}  # seconds per child


def resources() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
              "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_clust.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / SGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(ROOT, "mmvae_amd", "csrc", "kmeans.hip"), "-o", os.path.join(tmp, "dev.o")],
                             capture_output=True, text=True, check=True).stderr
    name, row, scratch = None, {}, 0
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
            scratch += int(row["VGPRs Spill"]) + int(row["ScratchSize [bytes/lane]"])
            name = None
    print("no kernel uses scratch memory (SGPR spills go to VGPR lanes)" if scratch == 0 else "SOME KERNEL USES SCRATCH MEMORY")
    return 0


def mixture(n, c, torch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + c)
    centres = 2.0 * torch.randn(c, D, device="cuda", generator=g)
    cluster = torch.randint(0, c, (n,), device="cuda", generator=g)
    return centres[cluster] + torch.randn(n, D, device="cuda", generator=g), cluster.to(torch.int32)


def torch_step(torch, x, cen, chunk=65536):
    """(new centroids, labels, dist2) of one Lloyd iteration in stock torch ops."""
    n, C = x.shape[0], cen.shape[0]
    label = torch.empty(n, dtype=torch.int64, device=x.device)
    d2 = torch.empty(n, dtype=torch.float32, device=x.device)
    for i0 in range(0, n, chunk):
        d, l = torch.cdist(x[i0:i0 + chunk], cen).min(1)
        label[i0:i0 + chunk] = l
        d2[i0:i0 + chunk] = d * d
    sums = torch.zeros_like(cen).index_add_(0, label, x)
    counts = torch.bincount(label, minlength=C)
    new = torch.where((counts > 0)[:, None], sums / counts.clamp_min(1)[:, None], cen)
    return new, label, d2


def child(n: int, host_rows: int, once: bool) -> int:
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        print("bench_kmeans: no GPU -- nothing is measured without one", file=sys.stderr)
        return 2
    from mmvae_amd import _clust_lib
    from mmvae_amd import clustering as K

    lib = _clust_lib.load_clust()

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

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for c in CLUSTERS:
        z, cluster = mixture(n, c, torch)
        z64 = z.double()
        x = (z64 - z64.mean(0, keepdim=True)).float().contiguous()
        del z64
        u = np.random.default_rng(0).random(c)
        cen = x[K.kmeans_seed(x, c, u).cuda()].contiguous()
        buf = K._StepBuffers(lib, n, D, c, x.device)
        new = torch.empty_like(cen)
        label = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        mind2 = torch.empty(n, dtype=torch.float32, device="cuda")
        print(f"\nN = {n}, D = {D}, C = {c} on {torch.cuda.get_device_name(0)}; workspace {buf.nbytes / 2 ** 20:.1f} MiB")
        legs = {"step": lambda: K._step_device(lib, x, D, cen, new, label, buf),
                "seed pass": lambda: K._seed_update(x, D, 5, True, mind2, True),
                "torch step": lambda: torch_step(torch, x, cen)}
        if once:  # one call of each entry, for a kernel trace
            legs["step"]()
            legs["seed pass"]()
            torch.cuda.synchronize()
            print("  one call of each entry made")
            continue
        reps = {}
        for name, fn in legs.items():  # warm-up, and the calls that fill 0.5 s
            fn()
            reps[name] = max(1, int(math.ceil(0.5 / max(clock(fn)[0], 1e-4))))
        times = {name: [] for name in legs}
        for _ in range(3):
            for name, fn in legs.items():
                times[name].append(events(fn, reps[name]))
        print("  3 alternating blocks of >= 0.5 s, device events, ms per call, the median block")
        floor = 4.0 * n * D
        for name in legs:
            t = med(times[name])
            line = f"    {name:12s} {t:10.3f} ms (blocks {' '.join(f'{v:.3f}' for v in times[name])}; {reps[name]} calls each)"
            if name != "torch step":
                line += f"   {floor / (t * 1e-3) / 1e12:6.3f} TB/s of the one read of x (4 N D = {floor / 1e6:.0f} MB)"
            if name == "step":
                line += f"; {2.0 * n * c * D / (t * 1e-3) / 1e12:5.1f} TFLOP/s of the N C D product"
            print(line)
        t_step, t_torch = med(times["step"]), med(times["torch step"])
        print(f"    torch step / step {t_torch / t_step:.2f} x ({'HIP is not slower' if t_step <= t_torch else 'HIP IS SLOWER'})")
        label.fill_(-1)
        legs["step"]()
        tn, tl, td = torch_step(torch, x, cen)
        torch.cuda.synchronize()
        print(f"    agreement with torch: {int((tl != label.long()).sum())} of {n} labels differ, centroids by at most "
              f"{float((tn - new).abs().max()):.2e}, dist2 by {float((td - buf.dist2).abs().max()):.2e} (largest "
              f"{float(buf.dist2.max()):.1f}); a second step call is bit-equal: ", end="")
        first = (new.clone(), buf.dist2.clone(), buf.stats.clone())
        label.fill_(-1)
        legs["step"]()
        torch.cuda.synchronize()
        print(all(torch.equal(a, b) for a, b in zip(first, (new, buf.dist2, buf.stats))))
        del tn, tl, td, first
        K.kmeans_fit(z, c)
        whole = [clock(lambda: K.kmeans_fit(z, c))[0] for _ in range(3)]
        fit = K.kmeans_fit(z, c)
        table = K.contingency(fit.labels, cluster, c, c)
        print(f"  kmeans_fit(z, {c}): {sorted(whole)[1]:.3f} s (calls {' '.join(f'{v:.3f}' for v in whole)}); {fit.n_iter} "
              f"iterations, converged {fit.converged}, inertia {fit.inertia:.6e}, ARI against the planted clusters "
              f"{K.adjusted_rand_index(table):.4f}, NMI {K.normalized_mutual_info(table):.4f}")
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            print("  scikit-learn is not importable here: the host figure is not measured")
            continue
        rows = min(host_rows, n)
        xs = z[:rows].cpu().numpy()
        t0 = time.perf_counter()
        km = KMeans(n_clusters=c, n_init=1, algorithm="lloyd", random_state=0).fit(xs)
        t_host = time.perf_counter() - t0
        print(f"  sklearn.cluster.KMeans(lloyd, n_init=1) on this host's CPU: {t_host:.3f} s for {rows} rows, {km.n_iter_} "
              f"iterations, inertia {km.inertia_:.6e} (measured)")
        del z, x, buf
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--host-rows", type=int, default=100_000, help="rows scikit-learn is timed on (at most 100 000)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.txt"))
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers, LDS and spills; no GPU")
    ap.add_argument("--once", type=int, help="one call of each entry at this N, in this process (for a kernel trace)")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    host_rows = min(args.host_rows, 100_000)
    if args.resources:
        return resources()
    if args.once:
        return child(args.once, host_rows, True)
    if args.child:
        return child(args.child, host_rows, False)
    lines, rc = [], 0
    for n in args.sizes:
        limit = LIMIT.get(n, 540)
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
