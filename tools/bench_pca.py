#!/usr/bin/env python3
"""The PCA moments and the principal-component regression (libmmvae_pca.so, mmvae_amd.pca), measured.

    python tools/bench_pca.py                  # on the GPU; the lines also go to --out (default profiles/pca.txt)
    python tools/bench_pca.py --resources      # no GPU: registers, LDS, scratch, spills and occupancy of the kernels

Data: a seeded mixture of 15 Gaussian clusters moved off the origin, at (N, D) = (100 000, 128), (1 000 000, 128),
(1 000 000, 50) and (100 000, 512).  One child process per shape, each under its own time limit (a child that faults,
aborts or runs out of time ends the run: nothing more is started on the device).  Per child, device events around blocks
of calls, the median of three blocks:

  scatter      mmvae_pca_scatter_f32 against the same definition in torch ops, (z - mean).T @ (z - mean) in fp32 and in
               fp64; TFLOP/s counted as the full product, 2 N D^2, against the 157 TFLOP/s fp32-MFMA peak; the largest
               error against the fp64 product, relative to the largest element, beside torch's fp32 product's
  class sums   mmvae_pca_group_sums_f64 at C = 2, 15 and 4 644 classes (the sort is not timed on either side) against
               zeros.index_add_(0, codes, (z - mean).double())
  projection   mmvae_pca_project_f32 at P = 2, 50 and D against (z - mean) @ V.T
  whole        pca.pca_fit and pca.pc_regression (three covariates: 2 and 4 644 classes and, below D = 512, a numeric one), host clock
               around a synchronised call; torch.pca_lowrank(q = 50) on the device; on the host (N = 100 000 only)
               sklearn's PCA(svd_solver="full") + LinearRegression on the dummies of the 2-class covariate

Nothing is asserted: the numbers are reported, and a row where an entry loses to torch says so.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(100_000, 128), (1_000_000, 128), (1_000_000, 50), (100_000, 512)]
CLUSTERS = 15
CLASSES = [2, 15, 4644]
PEAK_TFLOPS = 157.0
LIMIT = 420  # seconds per child


def resources() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
              "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_pca.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / SGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(ROOT, "mmvae_amd", "csrc", "pca_moments.hip"), "-o", os.path.join(tmp, "dev.o")],
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
            print(f"  {demangled.split('::')[-1]:28s} " + " / ".join(row[f] for f in fields))
            scratch += int(row["ScratchSize [bytes/lane]"])
            name = None
    print("no kernel uses scratch memory" if scratch == 0 else f"SCRATCH MEMORY IS USED: {scratch} bytes per lane in all")
    return 0 if scratch == 0 else 1


def child(n: int, d: int) -> int:
    import numpy as np
    import pandas as pd
    import torch

    if not torch.cuda.is_available():
        print("bench_pca: no GPU -- nothing is measured without one", file=sys.stderr)
        return 2
    from mmvae_amd import _pca_lib, pca

    lib = _pca_lib.load_pca()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

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
    blocks = lambda v: " ".join(f"{t:.3f}" for t in v)  # noqa: E731

    def versus(what, hip, stock, extra=""):
        verdict = "HIP is not slower" if med(hip) <= med(stock) else "HIP IS SLOWER"
        print(f"  {what}: HIP {med(hip):.3f} ms (blocks {blocks(hip)})   torch {med(stock):.3f} ms (blocks {blocks(stock)})   "
              f"torch / HIP {med(stock) / med(hip):.2f} x   {verdict}{extra}")

    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 2.0 * torch.randn(CLUSTERS, d, device="cuda", generator=g)
    cluster = torch.randint(0, CLUSTERS, (n,), device="cuda", generator=g)
    z = centres[cluster] + torch.randn(n, d, device="cuda", generator=g) + 3.0
    print(f"\nN = {n}, D = {d}, {CLUSTERS} clusters moved off the origin by 3 on {torch.cuda.get_device_name(0)}")
    mean = (pca.column_sums(z) / n).float()

    # ---- scatter
    nbytes = lib.mmvae_pca_scatter_workspace_bytes(n, d, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    S = torch.empty((d, d), dtype=torch.float64, device="cuda")

    def hip_scatter():
        lib.mmvae_pca_scatter_f32(n, d, z.data_ptr(), d, 0, None, 0, mean.data_ptr(), S.data_ptr(), ws.data_ptr(), nbytes,
                                  stream())

    def torch_scatter32():
        c = z - mean
        return c.T @ c

    def torch_scatter64():
        c = (z - mean).double()
        return c.T @ c

    hip_scatter()
    S32, S64 = torch_scatter32(), torch_scatter64()
    scale = float(S64.abs().max())
    err_hip, err_32 = float((S - S64).abs().max()) / scale, float((S32.double() - S64).abs().max()) / scale
    t_hip = [events(hip_scatter, 10) for _ in range(3)]
    t_32 = [events(torch_scatter32, 5) for _ in range(3)]
    t_64 = [events(torch_scatter64, 3) for _ in range(3)]
    tflops = 2.0 * n * d * d / (med(t_hip) * 1e-3) / 1e12
    versus("scatter", t_hip, t_32, f"; torch fp64 {med(t_64):.3f} ms (blocks {blocks(t_64)}), {med(t_64) / med(t_hip):.2f} x "
           f"HIP; HIP {tflops:.2f} TFLOP/s counted as 2 N D^2 = {100 * tflops / PEAK_TFLOPS:.1f} % of {PEAK_TFLOPS:.0f}; "
           f"workspace {nbytes / 2 ** 20:.1f} MiB; largest error against fp64 / largest element: HIP {err_hip:.2e}, "
           f"torch fp32 {err_32:.2e}; symmetric bit for bit: {bool(torch.equal(S, S.T))}")
    del S32, S64

    # ---- class sums
    nb = lib.mmvae_pca_group_sums_workspace_bytes(n, d)
    ws2 = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for C in CLASSES:
        codes = torch.randint(0, C, (n,), device="cuda", generator=g)
        order, run_ptr, _ = pca.sorted_classes(codes, C)
        sums = torch.empty((C, d), dtype=torch.float64, device="cuda")

        def hip_sums():
            lib.mmvae_pca_group_sums_f64(n, d, z.data_ptr(), d, mean.data_ptr(), C, order.data_ptr(), run_ptr.data_ptr(),
                                         sums.data_ptr(), ws2.data_ptr(), nb, stream())

        def torch_sums():
            return torch.zeros((C, d), dtype=torch.float64, device="cuda").index_add_(0, codes, (z - mean).double())

        hip_sums()
        want = torch_sums()
        rel = float((sums - want).abs().max()) / float(want.abs().max())
        t_hip = [events(hip_sums, 10) for _ in range(3)]
        t_stock = [events(torch_sums, 3) for _ in range(3)]
        t_sort, _ = clock(lambda: pca.sorted_classes(codes, C))
        versus(f"class sums, C = {C}", t_hip, t_stock, f"; the device sort and run_ptr (not in either figure) "
               f"{t_sort * 1e3:.3f} ms; differs from index_add_ by at most {rel:.1e} of the largest sum")
        del want

    # ---- projection
    for P in sorted({2, min(50, d), d}):
        V = torch.linalg.qr(torch.randn(d, P, device="cuda", generator=g))[0].T.contiguous()
        scores = torch.empty((n, P), dtype=torch.float32, device="cuda")

        def hip_project():
            lib.mmvae_pca_project_f32(n, d, z.data_ptr(), d, mean.data_ptr(), P, V.data_ptr(), scores.data_ptr(), P, stream())

        def torch_project():
            return (z - mean) @ V.T

        hip_project()
        rel = float((scores - torch_project()).abs().max()) / float(scores.abs().max())
        t_hip = [events(hip_project, 10) for _ in range(3)]
        t_stock = [events(torch_project, 5) for _ in range(3)]
        versus(f"projection, P = {P}", t_hip, t_stock, f"; differs from torch by at most {rel:.1e} of the largest score")

    # ---- the whole calls
    rng = np.random.default_rng(0)
    lab = cluster.cpu().numpy()
    metadata = pd.DataFrame({"species": np.where(rng.random(n) < 0.5, "human", "mouse"),
                             "donor": [f"d{i}" for i in rng.integers(0, 4644, n)],
                             "total_counts": (lab + rng.standard_normal(n)).astype(np.float32)})
    # (a numeric covariate is one more column of the scatter: at D = 512 there is no room for it)
    covariates = ("species", "donor", "total_counts") if d < 512 else ("species", "donor")
    pca.pca_fit(z)
    t_fit = [clock(lambda: pca.pca_fit(z))[0] for _ in range(3)]
    pca.pc_regression(z, metadata, covariates)
    t_pcr = [clock(lambda: pca.pc_regression(z, metadata, covariates))[0] for _ in range(3)]
    out = pca.pc_regression(z, metadata, covariates)
    torch.pca_lowrank(z, q=min(50, d))
    t_low = [clock(lambda: torch.pca_lowrank(z, q=min(50, d)))[0] for _ in range(3)]
    print(f"  pca_fit(z): {med(t_fit) * 1e3:.1f} ms (calls {blocks([t * 1e3 for t in t_fit])}); torch.pca_lowrank(z, q = "
          f"{min(50, d)}) {med(t_low) * 1e3:.1f} ms (calls {blocks([t * 1e3 for t in t_low])}); pc_regression(z, metadata, {len(covariates)} "
          f"covariates) {med(t_pcr) * 1e3:.1f} ms (calls {blocks([t * 1e3 for t in t_pcr])}), the factorising of the "
          f"metadata columns on the host included")
    print("  result: " + ", ".join(f"pcr({r.covariate}) = {r.pcr:.6f}" for r in out.summary.itertuples()))
    if n <= 100_000:
        try:
            from sklearn.decomposition import PCA
            from sklearn.linear_model import LinearRegression

            def host():
                X = z.cpu().numpy().astype(np.float64)
                fit = PCA(svd_solver="full").fit(X)
                scores = fit.transform(X)
                dummies = pd.get_dummies(metadata["species"]).to_numpy(dtype=np.float64)
                r2 = np.array([LinearRegression().fit(dummies, s).score(dummies, s) for s in scores.T])
                return float((fit.explained_variance_ * r2).sum() / fit.explained_variance_.sum())

            t_host, value = clock(host)
            print(f"  sklearn on this host's CPU: PCA(svd_solver='full') + LinearRegression per component, one covariate: "
                  f"{t_host:.2f} s, pcr(species) = {value:.6f} (the device's differs by {abs(value - out.pcr('species')):.1e})")
        except ImportError:
            print("  scikit-learn is not installed: no host figures")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=None, help="N D [N D ...]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca.txt"))
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers, LDS and spills; no GPU")
    ap.add_argument("--child", type=int, nargs=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.resources:
        return resources()
    if args.child:
        return child(*args.child)
    shapes = SHAPES if not args.shapes else list(zip(args.shapes[::2], args.shapes[1::2]))
    lines, rc = [], 0
    for n, d in shapes:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(d)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"[N = {n}, D = {d}] ran past its {LIMIT} s limit: stopping here")
            print(lines[-1])
            rc = 1
            break
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"[N = {n}, D = {d}] exited with {p.returncode}: stopping here\n{p.stderr[-2000:]}")
            print(lines[-1])
            rc = 1
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
