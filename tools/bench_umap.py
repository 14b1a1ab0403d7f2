#!/usr/bin/env python3
"""The UMAP of latent embeddings (libmmvae_umap.so, mmvae_amd.umap), measured.

Three legs, each in a child process of its own under its own time limit (a leg that faults, aborts or runs out of time
ends the run: nothing more is started on the device):

  knn        ms of mmvae_umap_knn_cosine_f32 (unit rows + Gram / top-k, both launches) at (N, D, k) = (100 000, 128, 30)
             and (20 000, 50, 15), device events around blocks of calls; the rate 2 N^2 D / time against the 157 TFLOP/s
             fp32-MFMA peak; and ms of the torch statement on the same device (normalise, chunked torch.matmul +
             torch.topk over 8192-row chunks), with the share of entries on which the two agree
  umap       s of the whole mmvae_amd.umap.umap_embeddings call (defaults: 200 epochs, pca start) on clustered data of
             the same two shapes, host clock around a synchronised call, and where the time goes by stage
  resources  registers, LDS, scratch and spills of every kernel of the library as the compiler reports them
             (-Rpass-analysis=kernel-resource-usage); needs hipcc, not a GPU

Nothing is asserted: the numbers are reported.  Output: the lines below, also written to --out (default
profiles/umap.txt; --append adds to it)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(100000, 128, 30), (20000, 50, 15)]
PEAK_F32_MFMA = 157e12
LEGS = {"knn": 300, "umap": 420, "resources": 300}  # seconds


def _clustered(N, D, seed=0):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = 2.0 * torch.randn(40, D, device="cuda", generator=g)
    which = torch.randint(0, 40, (N,), device="cuda", generator=g)
    return centres[which] + torch.randn(N, D, device="cuda", generator=g)


def _events(fn, reps):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def leg_knn():
    import torch

    from mmvae_amd import umap as U

    for N, D, k in SHAPES:
        x = torch.randn(N, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

        def ours():
            return U.knn_graph(x, k)

        def stock(chunk=8192):
            u = torch.nn.functional.normalize(x, dim=1)
            idx = torch.empty((N, k), dtype=torch.int64, device="cuda")
            dist = torch.empty((N, k), device="cuda")
            for r in range(0, N, chunk):
                top = torch.topk(u[r:r + chunk] @ u.T, k, dim=1, largest=True, sorted=True)
                idx[r:r + chunk], dist[r:r + chunk] = top.indices, 1.0 - top.values
            return idx, dist

        for fn in (ours, stock):  # code objects loaded, workspaces grown, algorithms picked
            fn()
            fn()
        torch.cuda.synchronize()
        reps = 3 if N >= 50000 else 10
        t_ours, t_stock = [], []
        for _ in range(3):  # interleaved blocks
            t_ours.append(_events(ours, reps))
            t_stock.append(_events(stock, reps))
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        agree = float((ours()[0][:, 1:].long() == stock()[0][:, 1:]).float().mean())
        flops = 2.0 * N * N * D
        print(f"kNN (N, D, k) = ({N}, {D}, {k}), 3 interleaved blocks of {reps} calls:")
        print(f"  mmvae_umap_knn_cosine_f32 : {med(t_ours):9.3f} ms   {flops / med(t_ours) / 1e9:7.1f} TFLOP/s = "
              f"{100 * flops / (med(t_ours) * 1e-3) / PEAK_F32_MFMA:5.1f} % of the fp32-MFMA peak   "
              f"(blocks {' '.join(f'{v:.3f}' for v in t_ours)})")
        print(f"  torch matmul + topk       : {med(t_stock):9.3f} ms   (blocks {' '.join(f'{v:.3f}' for v in t_stock)})")
        print(f"  torch / HIP               : {med(t_stock) / med(t_ours):9.2f} x   indices equal on {100 * agree:.2f} % "
              "of the ranks behind the point itself")


def leg_umap():
    import torch

    from mmvae_amd import umap as U

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for N, D, k in SHAPES:
        x = _clustered(N, D)
        U.umap_embeddings(x, n_neighbors=k)  # warm-up: code objects, workspaces
        whole = [clock(lambda: U.umap_embeddings(x, n_neighbors=k))[0] for _ in range(3)]
        t_knn, (idx, dist) = clock(lambda: U.knn_graph(x, k))
        t_set, graph = clock(lambda: U.fuzzy_simplicial_set(idx, dist))
        t_ab, (a, b) = clock(lambda: U.find_ab_params(1.0, 0.3))
        t_init, y0 = clock(lambda: U.initial_layout(x, 2, "pca", 0))
        t_prune, g = clock(lambda: U.layout_graph(graph, 200))
        t_lay, emb = clock(lambda: U.optimize_layout(y0, *g, n_epochs=200, a=a, b=b, seed=0))
        print(f"umap_embeddings (N, D, n_neighbors) = ({N}, {D}, {k}), 200 epochs, pca start, 2-D:")
        print(f"  whole call   : {sorted(whole)[1]:8.3f} s   (calls {' '.join(f'{v:.3f}' for v in whole)})")
        print(f"  by stage     : kNN {t_knn:.3f}  fuzzy set {t_set:.3f} (of it torch sort / unique: all but one launch)  "
              f"a, b fit {t_ab:.3f}  start {t_init:.3f}  prune {t_prune:.3f}  layout {t_lay:.3f} s")
        print(f"  graph        : {graph.indices.numel()} directed edges, {g[1].numel()} after pruning, longest row "
              f"{int((g[0][1:] - g[0][:-1]).max())}; embedding finite: {bool(torch.isfinite(emb).all())}")


def leg_resources():
    csrc = os.path.join(ROOT, "mmvae_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
              "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_umap.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("umap_knn.hip", "umap_layout.hip"):
            out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                                  "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, src), "-o",
                                  os.path.join(tmp, "dev.o")], capture_output=True, text=True, check=True).stderr
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
                    print(f"  {demangled.split('::')[-1]:28s} " + " / ".join(row[f] for f in fields))
                    name = None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default="knn,umap,resources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umap.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        {"knn": leg_knn, "umap": leg_umap, "resources": leg_resources}[args.leg]()
        return 0
    lines = []
    for leg in args.legs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True,
                               timeout=LEGS[leg])
        except subprocess.TimeoutExpired:
            lines.append(f"[{leg}] ran past its {LEGS[leg]} s limit: stopping here")
            print(lines[-1])
            break
        sys.stdout.write(p.stdout)
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"[{leg}] exited with {p.returncode}: stopping here\n{p.stderr[-2000:]}")
            print(lines[-1])
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
