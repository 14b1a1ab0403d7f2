#!/usr/bin/env python3
"""Connected components, component sizes and kBET on the latent kNN graph (libmmvae_graph.so, mmvae_amd.graph_metrics),
measured.

    python tools/bench_graph.py                  # on the GPU; the lines also go to --out (default profiles/graph.txt)
    python tools/bench_graph.py --resources      # no GPU: registers, LDS, scratch, spills and occupancy of the kernels

Data: a seeded mixture of 15 Gaussian clusters in 128 dimensions, two batches, the cluster as the label, at N = 100 000
and 1 000 000 cells and k = 15 and 64.  One child process per (size, k), each under its own time limit (a child that
faults, aborts or runs out of time ends the run: nothing more is started on the device).  Per child:

  components   graph_metrics.connected_components with the labels as codes: rounds, ms per round (device events around
               mmvae_graph_cc_round_i32 calls from parent = arange) and the whole call with its read-back per round
  sizes        ms of mmvae_graph_component_sizes_i32
  kbet         ms of mmvae_graph_kbet_f64
  torch        the same definitions in torch ops on the same device: scatter_reduce(amin) sweeps with parent[parent] and
               bincounts (graph_metrics._components_torch; sizes by bincount and scatter_reduce(amax)); one-hot counts
               and torch.special.gammaincc
  scipy        scipy.sparse.csgraph.connected_components and scipy.stats.chi2.sf on this host's CPU, the copies to the
               host included
  whole        s of graph_metrics.graph_metrics(z, metadata), host clock around a synchronised call, kNN and the rest

Nothing is asserted: the numbers are reported.
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

SIZES = [100_000, 1_000_000]
KS = [15, 64]
D, CLUSTERS = 128, 15
LIMIT = {100_000: 300, 1_000_000: 600}  # seconds per child


def resources() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
              "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_graph.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / SGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(ROOT, "mmvae_amd", "csrc", "graph_cc.hip"), "-o", os.path.join(tmp, "dev.o")],
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
            print(f"  {demangled.split('::')[-1]:24s} " + " / ".join(row[f] for f in fields))
            scratch += int(row["ScratchSize [bytes/lane]"])
            name = None
    print("no kernel uses scratch memory" if scratch == 0 else f"SCRATCH MEMORY IS USED: {scratch} bytes per lane in all")
    return 0 if scratch == 0 else 1


def mixture(n, torch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = 2.0 * torch.randn(CLUSTERS, D, device="cuda", generator=g)
    cluster = torch.randint(0, CLUSTERS, (n,), device="cuda", generator=g)
    batch = torch.randint(0, 2, (n,), device="cuda", generator=g)
    z = centres[cluster] + torch.randn(n, D, device="cuda", generator=g)
    return z, batch.to(torch.int32), cluster.to(torch.int32)


def child(n: int, k: int) -> int:
    import numpy as np
    import pandas as pd
    import torch

    if not torch.cuda.is_available():
        print("bench_graph: no GPU -- nothing is measured without one", file=sys.stderr)
        return 2
    from mmvae_amd import _graph_lib
    from mmvae_amd import graph_metrics as G
    from mmvae_amd import umap as U

    lib = _graph_lib.load_graph()
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
    z, batch, label = mixture(n, torch)
    idx, _ = U.knn_graph(z, k)
    print(f"\nN = {n}, k = {k}, D = {D}, {CLUSTERS} clusters (the codes), 2 batches on {torch.cuda.get_device_name(0)}")

    # ---- components
    root, rounds = G.connected_components(idx, label, _trusted=True)
    conn = G.graph_connectivity(idx, label, CLUSTERS, _trusted=True)
    parent = torch.empty(n, dtype=torch.int32, device="cuda")
    changed = torch.zeros(1, dtype=torch.int32, device="cuda")
    start = torch.arange(n, dtype=torch.int32, device="cuda")

    def hip_rounds():
        parent.copy_(start)
        for _ in range(rounds):
            lib.mmvae_graph_cc_round_i32(n, k, idx.data_ptr(), label.data_ptr(), parent.data_ptr(), changed.data_ptr(),
                                         stream())

    hip_rounds()
    t_rounds = [events(hip_rounds, 5) for _ in range(3)]
    t_call = [clock(lambda: G.connected_components(idx, label, _trusted=True))[0] * 1e3 for _ in range(5)]
    t_torch = [clock(lambda: G._components_torch(idx, label, G.MAX_ROUNDS))[0] * 1e3 for _ in range(3)]
    troot, trounds = G._components_torch(idx, label, G.MAX_ROUNDS)
    print(f"  components: {conn.n_components} components, connectivity {conn.score:.6f}; HIP {rounds} rounds, "
          f"{med(t_rounds) / rounds:.3f} ms per round ({med(t_rounds):.3f} ms for all, blocks "
          f"{' '.join(f'{v:.3f}' for v in t_rounds)}), the whole call with one read-back per round {med(t_call):.3f} ms "
          f"(calls {' '.join(f'{v:.3f}' for v in t_call)})")
    verdict = "HIP is not slower" if med(t_call) <= med(t_torch) else "HIP IS SLOWER"
    print(f"  components, torch ops on the device: {trounds} rounds, {med(t_torch):.3f} ms (calls "
          f"{' '.join(f'{v:.3f}' for v in t_torch)}); torch / HIP {med(t_torch) / med(t_call):.2f} x   {verdict}; "
          f"roots equal: {bool(torch.equal(troot, root))}")
    del troot

    # ---- sizes
    size_ws = torch.empty(n, dtype=torch.int32, device="cuda")
    count = torch.empty(CLUSTERS, dtype=torch.int64, device="cuda")
    largest = torch.empty(CLUSTERS, dtype=torch.int32, device="cuda")
    n_comp = torch.empty(1, dtype=torch.int32, device="cuda")

    def hip_sizes():
        lib.mmvae_graph_component_sizes_i32(n, root.data_ptr(), label.data_ptr(), CLUSTERS, size_ws.data_ptr(),
                                            count.data_ptr(), largest.data_ptr(), n_comp.data_ptr(), stream())

    def torch_sizes():
        c, r = label.long(), root.long()
        ok = c >= 0
        cnt = torch.bincount(c[ok], minlength=CLUSTERS)
        size = torch.bincount(r[ok], minlength=n)
        is_root = ok & (r == torch.arange(n, device="cuda"))
        big = torch.zeros(CLUSTERS, dtype=torch.int64, device="cuda").scatter_reduce(0, c[is_root], size[is_root], "amax")
        return cnt, big, is_root.sum()

    hip_sizes()
    tc, tb, tn = torch_sizes()
    same = bool(torch.equal(tc, count) and torch.equal(tb.to(torch.int32), largest) and int(tn) == int(n_comp))
    t_hip = [events(hip_sizes, 20) for _ in range(3)]
    t_stock = [events(torch_sizes, 5) for _ in range(3)]
    verdict = "HIP is not slower" if med(t_hip) <= med(t_stock) else "HIP IS SLOWER"
    print(f"  component sizes: HIP {med(t_hip):.3f} ms (blocks {' '.join(f'{v:.3f}' for v in t_hip)})   torch "
          f"{med(t_stock):.3f} ms (blocks {' '.join(f'{v:.3f}' for v in t_stock)})   torch / HIP "
          f"{med(t_stock) / med(t_hip):.2f} x   {verdict}; results equal: {same}")

    # ---- kBET
    freq = G.batch_frequencies(batch, 2)
    freq_d = freq.cuda()
    stat = torch.empty(n, dtype=torch.float64, device="cuda")
    pval = torch.empty_like(stat)

    def hip_kbet():
        lib.mmvae_graph_kbet_f64(n, k, idx.data_ptr(), batch.data_ptr(), 2, freq_d.data_ptr(), 1, stat.data_ptr(),
                                 pval.data_ptr(), stream())

    def torch_kbet():
        bj = batch[idx[:, 1:].long()]
        counts = torch.nn.functional.one_hot(bj.long(), 2).sum(1).double()
        e = counts.sum(1, keepdim=True) * freq_d
        s = ((counts - e) ** 2 / e).sum(1)
        return s, torch.special.gammaincc(torch.full_like(s, 0.5), 0.5 * s)

    hip_kbet()
    ts, tp = torch_kbet()
    rel = float(((tp - pval).abs() / pval).nan_to_num(0.0).max())
    t_hip = [events(hip_kbet, 20) for _ in range(3)]
    t_stock = [events(torch_kbet, 5) for _ in range(3)]
    verdict = "HIP is not slower" if med(t_hip) <= med(t_stock) else "HIP IS SLOWER"
    print(f"  kBET: HIP {med(t_hip):.3f} ms (blocks {' '.join(f'{v:.3f}' for v in t_hip)})   torch "
          f"{med(t_stock):.3f} ms (blocks {' '.join(f'{v:.3f}' for v in t_stock)})   torch / HIP "
          f"{med(t_stock) / med(t_hip):.2f} x   {verdict}; rejection rate {G.rejection_rate(pval):.4f}, p differs from "
          f"torch.special.gammaincc by at most {rel:.2e} relative")
    del ts, tp

    # ---- scipy on the host
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
        from scipy.stats import chi2

        def host_cc():
            i, c = idx.cpu().numpy(), label.cpu().numpy()
            src = np.repeat(np.arange(n), k)
            dst = i.reshape(-1)
            keep = (c[src] >= 0) & (c[src] == c[dst])
            g = sp.coo_matrix((np.ones(int(keep.sum()), dtype=np.int8), (src[keep], dst[keep])), shape=(n, n))
            return connected_components(g, directed=False)[0]

        t_cc, n_host = clock(host_cc)
        t_chi, _ = clock(lambda: chi2.sf(stat.cpu().numpy(), 1))
        print(f"  scipy on this host's CPU: csgraph.connected_components {t_cc * 1e3:.1f} ms ({n_host} components, the copy "
              f"of idx and the CSR build included; {t_cc * 1e3 / med(t_call):.1f} x the HIP call), chi2.sf of the device's "
              f"stat {t_chi * 1e3:.1f} ms")
    except ImportError:
        print("  scipy is not installed: no host figures")

    # ---- the whole call
    names = [f"type{i:02d}" for i in range(CLUSTERS)]
    lab, bat = label.cpu().numpy(), batch.cpu().numpy()
    metadata = pd.DataFrame({"species": ["human" if b == 0 else "mouse" for b in bat], "cell_type": [names[c] for c in lab]})
    G.graph_metrics(z, metadata, n_neighbors=k)
    whole = [clock(lambda: G.graph_metrics(z, metadata, n_neighbors=k))[0] for _ in range(3)]
    t_knn, _ = clock(lambda: U.knn_graph(z, k))
    t_per, per = clock(lambda: G.kbet_per_label(z, batch, label, n_labels=CLUSTERS, n_batches=2))
    out = G.graph_metrics(z, metadata, n_neighbors=k)
    row = out.summary.iloc[0]
    print(f"  graph_metrics(z, metadata, n_neighbors={k}): {sorted(whole)[1]:.3f} s (calls "
          f"{' '.join(f'{v:.3f}' for v in whole)}); of it the kNN graph {t_knn:.3f} s, kbet_per_label (15 graphs of 64 "
          f"neighbours and their tests) {t_per:.3f} s, the rest {sorted(whole)[1] - t_knn - t_per:.3f} s")
    print(f"  result: graph connectivity {row['graph_connectivity']:.6f}, {row['n_components']} components in "
          f"{row['cc_rounds']} rounds, kBET rejection whole graph {row['kbet_rejection_global']:.4f}, per-label score "
          f"{row['kbet_score']:.4f}")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--ks", type=int, nargs="+", default=KS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph.txt"))
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers, LDS and spills; no GPU")
    ap.add_argument("--child", type=int, nargs=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.resources:
        return resources()
    if args.child:
        return child(*args.child)
    lines, rc = [], 0
    for n in args.sizes:
        for k in args.ks:
            limit = LIMIT.get(n, 600)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(k)],
                                   capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                lines.append(f"[N = {n}, k = {k}] ran past its {limit} s limit: stopping here")
                print(lines[-1])
                rc = 1
                break
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            lines += p.stdout.splitlines()
            if p.returncode != 0:
                lines.append(f"[N = {n}, k = {k}] exited with {p.returncode}: stopping here\n{p.stderr[-2000:]}")
                print(lines[-1])
                rc = 1
                break
        if rc:
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
