#!/usr/bin/env python3
"""The count normalisation (libmmvae_prep.so, ops.csr_log1p_normalize_, SpeciesChunks(normalize="log1p_cpm")), measured.

Three legs, each in a child process of its own under its own time limit (a leg that faults, aborts or runs out of time
ends the run: nothing more is started on the device):

  entry      us of one mmvae_prep_csr_log1p_norm_i32 launch (values in place + row sums) over a synthetic raw chunk of
             131 072 cells at 20 000 and at 60 530 genes, device events around blocks of calls, and GB/s of the 8 B per
             stored element the kernel must move.  Row lengths are drawn like synthetic.py's counts (a gene is stored with
             probability 1 - exp(-lambda_g), lambda_g = 0.15 LogNormal(0, 1); the row's length by the normal approximation
             of that sum), values are 1 + Poisson(0.3).  Repeated calls run on the output of the one before: the traffic
             is the same.  Beside it: a torch statement on the same device (segment_reduce, repeat_interleave, multiply,
             divide, log1p, copy back) and the reference's per-row numpy loop (normalize_data's getrow() loop, restated) on
             the first 2 000 rows on the host, EXTRAPOLATED to the chunk by the row count
  feed       tools/bench_feed.py --device-chunks 1 with --normalize 0 (pre-normalised files: the behaviour before) and
             --normalize 1 (raw files, normalised behind the upload), alternating, one process per run
  resources  registers, LDS, scratch and spills of the library's kernels as the compiler reports them
             (-Rpass-analysis=kernel-resource-usage); needs hipcc, not a GPU

Nothing is asserted: the numbers are reported, with the two comparisons the normalisation must win or hold spelled out.
Output: the lines below, also written to --out (default profiles/prep.txt; --append adds to it)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ROWS = 131072
GENE_COUNTS = [20000, 60530]
HOST_ROWS = 2000
LEGS = {"entry": 420, "feed": 600, "resources": 120}  # seconds


def _events(fn, reps):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps * 1e3  # us


def _raw_chunk(G, seed):
    """(crow int32 [N_ROWS + 1], values fp32 [nnz]) on the device."""
    import torch

    g = torch.Generator().manual_seed(seed)
    lam = 0.15 * torch.exp(torch.randn(G, generator=g))
    p = 1.0 - torch.exp(-lam.double())
    mean, std = float(p.sum()), float((p * (1.0 - p)).sum().sqrt())
    gd = torch.Generator(device="cuda").manual_seed(seed)
    lengths = (mean + std * torch.randn(N_ROWS, device="cuda", generator=gd)).round().clamp_(1, G).to(torch.int64)
    crow = torch.zeros(N_ROWS + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lengths, 0, out=crow[1:])
    nnz = int(crow[-1])
    assert nnz <= 0x7fffffff
    values = 1.0 + torch.poisson(torch.full((nnz,), 0.3, device="cuda"), generator=gd)
    return crow.to(torch.int32), lengths, values


def host_loop(matrix):
    """The reference's normalize_data, restated: one getrow() per cell."""
    import numpy as np

    for row in range(matrix.shape[0]):
        a, b = matrix.indptr[row], matrix.indptr[row + 1]
        row_data = matrix.getrow(row).data
        matrix.data[a:b] = np.log1p((row_data * 1e4) / row_data.sum())


def leg_entry():
    import gc

    import scipy.sparse as sp
    import torch

    from mmvae_amd import ops

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for G in GENE_COUNTS:
        crow, lengths, values = _raw_chunk(G, seed=G)
        nnz = values.numel()
        sums = torch.empty(N_ROWS, dtype=torch.float32, device="cuda")
        n_head = int(crow[HOST_ROWS])  # (column indices: any distinct ones per row; the normalisation never reads them)
        head = sp.csr_matrix((values[:n_head].cpu().numpy(), (torch.arange(n_head, dtype=torch.int64) % G).to(torch.int32).numpy(),
                              crow[:HOST_ROWS + 1].cpu().numpy()), shape=(HOST_ROWS, G))
        traffic = 8.0 * nnz + 4.0 * (N_ROWS + 1) + 4.0 * N_ROWS

        def ours():
            ops.csr_log1p_normalize_(crow, values, 1e4, sums)

        def torch_statement():
            s = torch.segment_reduce(values, "sum", lengths=lengths)
            values.copy_(torch.log1p(values * 1e4 / torch.repeat_interleave(s, lengths)))

        print(f"raw chunk of {N_ROWS} cells x {G} genes: {nnz} stored elements ({nnz / N_ROWS:.0f} per cell, "
              f"{int(lengths.min())} .. {int(lengths.max())}), {4 * nnz / 1e6:.0f} MB of values")
        for _ in range(2):
            ours()
            torch_statement()
        torch.cuda.synchronize()
        reps = 10 if G <= 20000 else 5
        t_ours, t_torch = [], []
        for _ in range(3):  # interleaved blocks
            t_ours.append(_events(ours, reps))
            t_torch.append(_events(torch_statement, max(reps // 2, 2)))
        t0 = time.perf_counter()
        host_loop(head)
        t_host = (time.perf_counter() - t0) * 1e6 * (N_ROWS / HOST_ROWS)
        print(f"  mmvae_prep_csr_log1p_norm_i32                : {med(t_ours):10.1f} us   {8.0 * nnz / med(t_ours) / 1e3:7.1f} GB/s of 8 B per "
              f"element ({traffic / med(t_ours) / 1e3:.1f} with row pointers and sums)   (blocks {' '.join(f'{v:.1f}' for v in t_ours)})")
        print(f"  torch segment_reduce + repeat_interleave, dev : {med(t_torch):10.1f} us   {med(t_torch) / med(t_ours):7.1f} x   "
              f"(blocks {' '.join(f'{v:.1f}' for v in t_torch)})")
        print(f"  per-row numpy loop, host, {HOST_ROWS} rows EXTRAPOLATED : {t_host:10.0f} us   {t_host / med(t_ours):7.0f} x   "
              f"({t_host / 1e6 * HOST_ROWS / N_ROWS:.3f} s measured for {HOST_ROWS} rows)")
        print(f"  the entry is {'FASTER' if med(t_ours) < med(t_torch) else 'NOT FASTER'} than the torch statement at {G} genes")
        del crow, lengths, values, sums, head
        gc.collect()
        torch.cuda.empty_cache()


def leg_feed():
    tool = os.path.join(ROOT, "tools", "bench_feed.py")
    runs = {0: [], 1: []}
    for norm in (0, 1, 0, 1, 0, 1):
        p = subprocess.run([sys.executable, tool, "--device-chunks", "1", "--normalize", str(norm)], capture_output=True,
                           text=True, timeout=150)
        if p.returncode != 0:
            print(f"bench_feed --normalize {norm} exited with {p.returncode}: stopping here\n{p.stderr[-1500:]}")
            sys.exit(1)
        runs[norm].append(json.loads(p.stdout.strip().splitlines()[-1]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print("tools/bench_feed.py --device-chunks 1 (C2, batch 512, 400 steps behind 50 of warm-up), runs alternating, one process each:")
    rate = {}
    for norm, label in ((0, "normalize off, pre-normalised files"), (1, "normalize on, raw count files      ")):
        ms = [r["ms_per_step"] for r in runs[norm]]
        rate[norm] = med([1e3 / v for v in ms])
        print(f"  {label}: {med(ms):.4f} ms/step   {rate[norm]:.1f} batches/s   (runs {' '.join(f'{v:.4f}' for v in ms)})")
        for r in runs[norm]:
            print(f"      last losses {' '.join(f'{k.split(chr(47))[-1]} {v:.1f}' for k, v in sorted(r['last_losses'].items()))}")
    delta = 100.0 * (rate[1] / rate[0] - 1.0)
    print(f"  on against off: {delta:+.2f} % batches/s: {'inside' if abs(delta) <= 3.0 else 'OUTSIDE'} the box-to-box +-3 %")


def leg_resources():
    csrc = os.path.join(ROOT, "mmvae_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
              "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_prep.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "csr_prep.hip"), "-o",
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
                print(f"  {demangled.split('::')[-1]:36s} " + " / ".join(row[f] for f in fields))
                name = None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default="entry,feed,resources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        {"entry": leg_entry, "feed": leg_feed, "resources": leg_resources}[args.leg]()
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
