#!/usr/bin/env python3
"""The gradient histograms (libmmvae_hist.so, HipAdam.grad_histograms, record_gradients), measured.

Three legs, each in a child process of its own under its own time limit (a leg that faults, aborts or runs out of time
ends the run: nothing more is started on the device):

  arena      us of HipAdam.grad_histograms() over one expert's gradient arena (memsets, item pass and segment reduction;
             TensorBoard's 1 549 default edges) of the two-modality model at C2 size (20 000 genes) and at the
             reference's gene count (60 530), device events around blocks of calls, and arena bytes / time.  Three
             fillings: (a) the gradient real training steps on the seeded synthetic data left, (b) all zeros, (c)
             log-uniform magnitudes with both signs.  Beside it, on filling (a): the reference's way (per parameter
             .cpu().numpy() + np.histogram, host clock) and a torch composition on the device (per parameter
             torch.bucketize against the fp32-rounded edges + bincount + min / max / sum / sum of squares)
  step       ms of a C2 training step through the captured engine with every step recorded (interval 1, no logger) next
             to an unrecorded one, host clock around synchronised blocks of steps, blocks interleaved
  resources  registers, LDS, scratch and spills of the library's kernels as the compiler reports them
             (-Rpass-analysis=kernel-resource-usage); needs hipcc, not a GPU

Nothing is asserted: the numbers are reported.  Output: the lines below, also written to --out (default
profiles/gradhist.txt; --append adds to it)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENE_COUNTS = [20000, 60530]
LEGS = {"arena": 390, "step": 240, "resources": 120}  # seconds


def _events(fn, reps):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps * 1e3  # us


def _trained_model(G, steps, B=512, **settings):
    import pandas as pd
    import torch

    from mmvae_amd import rng, synthetic

    genes = {"human": G, "mouse": G}
    model = synthetic.build_model(genes, seed=0).cuda()
    torch.manual_seed(0)
    rng.reseed()
    for k, v in settings.items():
        setattr(model, k, v)
    model.train()
    model.trainer.set_stage("training")
    xs = {eid: synthetic.synthetic_counts(B, g, seed=1234 + i, device="cuda") for i, (eid, g) in enumerate(genes.items())}
    md = pd.DataFrame({"dummy": [0] * B})

    def step(i):
        eid = ("human", "mouse")[i % 2]
        model.trainer.global_step = i
        model.training_step((xs[eid], md, eid), i)

    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    return model, step


def leg_arena():
    import numpy as np
    import torch

    from mmvae_amd.histogram import tensorboard_edges

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    edges = tensorboard_edges()
    edges32 = torch.from_numpy(edges.astype(np.float32)).cuda()
    for G in GENE_COUNTS:
        model, _ = _trained_model(G, steps=5)  # (step 4 is human's third: a replay of its captured program)
        model._flush_engine()
        opt = model.get_optimizers()["experts"]["human"]
        a = opt.arena
        nbytes = 4 * a.numel
        real = a.grad.clone()
        g = torch.Generator(device="cuda").manual_seed(5)
        mag = 10.0 ** (torch.rand(a.numel, device="cuda", generator=g) * 12.0 - 10.0)
        spread = mag * (torch.randint(0, 2, (a.numel,), device="cuda", generator=g).float() * 2.0 - 1.0)
        del mag

        def ours():
            return opt.grad_histograms()

        def torch_device():
            out = []
            for i in range(len(a.params)):
                v = a.grad_view(i).reshape(-1)
                idx = torch.bucketize(v, edges32, right=True)
                out.append((torch.bincount(idx, minlength=edges32.numel() + 1), v.min(), v.max(), v.sum(), (v * v).sum()))
            return out

        def host_way():
            t0 = time.perf_counter()
            for i in range(len(a.params)):
                np.histogram(a.grad_view(i).cpu().numpy(), bins=edges)
            return (time.perf_counter() - t0) * 1e6

        zero_share = float((real == 0).float().mean())
        print(f"expert arena at {G} genes: {a.numel} fp32 gradients ({nbytes / 1e6:.1f} MB) in {len(a.params)} parameters, "
              f"{100 * zero_share:.1f} % exact zeros after real steps; 1549 edges")
        reps = 20 if G <= 20000 else 8
        rows = {}
        for name, fill in (("(a) real gradient", real), ("(b) all zeros", None), ("(c) log-uniform, both signs", spread)):
            a.grad.zero_() if fill is None else a.grad.copy_(fill)
            for _ in range(3):  # code object loaded, tables cached
                ours()
            torch.cuda.synchronize()
            blocks = [_events(ours, reps) for _ in range(3)]
            rows[name] = med(blocks)
            print(f"  grad_histograms {name:28s}: {med(blocks):9.1f} us   {nbytes / med(blocks) / 1e3:7.1f} GB/s of arena   "
                  f"(blocks {' '.join(f'{v:.1f}' for v in blocks)})")
        print(f"  (b) / (c)                                   : {rows['(b) all zeros'] / rows['(c) log-uniform, both signs']:9.2f} x")
        a.grad.copy_(real)
        for _ in range(2):
            torch_device()
        torch.cuda.synchronize()
        t_ours, t_torch = [], []
        for _ in range(3):  # interleaved blocks
            t_ours.append(_events(ours, reps))
            t_torch.append(_events(torch_device, max(reps // 4, 2)))
        t_host = [host_way() for _ in range(2 if G <= 20000 else 1)]
        print(f"  on (a): grad_histograms                     : {med(t_ours):9.1f} us   (blocks {' '.join(f'{v:.1f}' for v in t_ours)})")
        print(f"  on (a): torch bucketize + bincount, device  : {med(t_torch):9.1f} us   {med(t_torch) / med(t_ours):7.1f} x   "
              f"(blocks {' '.join(f'{v:.1f}' for v in t_torch)})")
        print(f"  on (a): .cpu().numpy() + np.histogram, host : {min(t_host):9.0f} us   {min(t_host) / med(t_ours):7.0f} x   "
              f"(calls {' '.join(f'{v:.0f}' for v in t_host)})")
        del model, opt, a, real, spread
        import gc

        gc.collect()
        torch.cuda.empty_cache()


def leg_step():
    import torch

    def clock(step, first, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(first, first + n):
            step(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    G, n = 20000, 100
    plain, step_plain = _trained_model(G, steps=20)
    rec, step_rec = _trained_model(G, steps=20, record_gradients=True, save_gradients_interval=1, gradient_record_cap=10 ** 6)
    t_plain, t_rec, at = [], [], 20
    for _ in range(3):  # interleaved blocks
        t_plain.append(clock(step_plain, at, n))
        t_rec.append(clock(step_rec, at, n))
        at += n
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print(f"C2 training step (2 x {G} genes, batch 512, captured engine, host clock over blocks of {n} steps):")
    print(f"  record_gradients off          : {med(t_plain):7.3f} ms   (blocks {' '.join(f'{v:.3f}' for v in t_plain)})")
    print(f"  every step recorded, no logger: {med(t_rec):7.3f} ms   (blocks {' '.join(f'{v:.3f}' for v in t_rec)})")
    print(f"  a recorded step costs         : {med(t_rec) - med(t_plain):7.3f} ms more: two histogram passes (VAE, expert), two "
          f"synchronising copies, {len(rec.gradient_histograms)} raw dictionaries built on the host")


def leg_resources():
    csrc = os.path.join(ROOT, "mmvae_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
              "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_hist.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "seg_hist.hip"), "-o",
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
    ap.add_argument("--legs", default="arena,step,resources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradhist.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        {"arena": leg_arena, "step": leg_step, "resources": leg_resources}[args.leg]()
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
