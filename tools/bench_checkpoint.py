#!/usr/bin/env python3
"""The checkpoint snapshot (libmmvae_ckpt.so, mmvae_amd.checkpoint, Trainer callbacks), measured.

Legs, each in a child process of its own under its own time limit (a leg that faults, aborts or runs out of time ends the
run: nothing more is started on the device):

  entry      us and TB/s (bytes read + bytes written) of one mmvae_ckpt_snapshot launch over the whole job table of the
             C2 model (two experts of 20 000 genes) and of the model at 60 530 / 52 437 genes, device events around
             blocks of calls; the digest-only mode (bytes read); beside it a plain torch `copy_` of the same arenas into
             the same private buffer (what the digest costs on top of a copy) and the clone-based `state_dict()` of the
             model and its optimisers on the device.  The fraction of the 6.29 TB/s float4-copy rate is printed.
  loop       200 steps of the C2 step through Trainer.fit (batch 512, two modalities in turn), three ways: without
             checkpoints; with the blocking `state_dict()` + torch.save every 50 steps; with ModelCheckpoint(
             every_n_train_steps=50) on the snapshot path.  Per way: mean and maximum host time of a step and the wall
             time of the loop, device drained.  `--variants none` runs on a tree from before the feature as well (it uses
             nothing of it): the comparison that a loop without checkpoints does not pay for them.
  resources  registers, LDS, scratch and spills of the library's kernels as the compiler reports them; needs hipcc, not a GPU

Nothing is asserted: the numbers are reported.  Output: the lines below, also written to --out (default
profiles/checkpoint.txt; --append adds to it)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12  # bytes / s: the measured float4 copy rate of the MI355X (read + written)
MODELS = [("C2", {"human": 20000, "mouse": 20000}), ("60 530 / 52 437 genes", {"human": 60530, "mouse": 52437})]
LEGS = {"entry": 420, "loop": 600, "resources": 120}  # seconds
STEPS, EVERY, BATCH = 200, 50, 512


def _events(fn, reps):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps * 1e3  # us


def leg_entry():
    import copy
    import gc

    import torch

    from mmvae_amd import synthetic
    from mmvae_amd.checkpoint import Checkpointer

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for label, genes in MODELS:
        model = synthetic.build_model(genes).cuda()
        model.optimizers()
        ck = Checkpointer(model)
        words = sum(r.n_words for r in ck.ranges)
        print(f"{label}: {len(ck.ranges)} ranges, {words} words ({4 * words / 1e9:.3f} GB), longest {ck.max_words}; floor "
              f"{8 * words / COPY_RATE * 1e6:.0f} us at {COPY_RATE / 1e12:.2f} TB/s")

        def snapshot():
            ck.launch()

        def digest_only():
            ck.launch(copy_out=False)

        views = [(ck.copy_dev[r.dst_word:r.dst_word + r.n_words], r.tensor.reshape(-1).view(torch.int32)) for r in ck.ranges
                 if r.n_words]

        def torch_copy():
            for d, s in views:
                d.copy_(s)

        def clones():
            return model.state_dict(), [copy.deepcopy(o.state_dict()) for o in model.optimizers()]

        for fn in (snapshot, digest_only, torch_copy, clones):
            fn()
        torch.cuda.synchronize()
        t = {"snap": [], "dig": [], "copy": [], "clone": []}
        for _ in range(3):  # interleaved blocks
            t["snap"].append(_events(snapshot, 10))
            t["dig"].append(_events(digest_only, 10))
            t["copy"].append(_events(torch_copy, 10))
            t["clone"].append(_events(clones, 3))
        blocks = lambda k: " ".join(f"{v:.1f}" for v in t[k])  # noqa: E731
        rate = 8.0 * words / med(t["snap"]) * 1e6
        print(f"  mmvae_ckpt_snapshot, copy + digest : {med(t['snap']):9.1f} us   {rate / 1e12:5.2f} TB/s read + written   "
              f"{100 * rate / COPY_RATE:5.1f} % of the copy rate   (blocks {blocks('snap')})")
        print(f"  mmvae_ckpt_snapshot, digest only   : {med(t['dig']):9.1f} us   {4.0 * words / med(t['dig']) * 1e6 / 1e12:5.2f} TB/s read"
              f"                                      (blocks {blocks('dig')})")
        rate_c = 8.0 * words / med(t["copy"]) * 1e6
        print(f"  torch copy_ of the same ranges     : {med(t['copy']):9.1f} us   {rate_c / 1e12:5.2f} TB/s   the digest costs "
              f"{med(t['snap']) - med(t['copy']):+.1f} us on top   (blocks {blocks('copy')})")
        print(f"  state_dict() + clones, on device   : {med(t['clone']):9.1f} us   {med(t['clone']) / med(t['snap']):5.1f} x   "
              f"(blocks {blocks('clone')})")
        del model, ck, views
        gc.collect()
        torch.cuda.empty_cache()


def _loop(variant, out_dir):
    import copy

    import pandas as pd
    import torch

    from mmvae_amd import synthetic
    from mmvae_amd.trainer import MultiModalBatches, Trainer

    genes = MODELS[0][1]
    model = synthetic.build_model(genes).cuda()
    md = pd.DataFrame({"dummy": [0] * BATCH})
    loaders = {eid: [(synthetic.synthetic_counts(BATCH, g, seed=1 + i, device="cuda"), md, eid)] * (STEPS // 2 + 25)
               for i, (eid, g) in enumerate(genes.items())}
    kw = {}
    if variant == "snapshot":
        from mmvae_amd.callbacks import ModelCheckpoint

        kw["callbacks"] = [ModelCheckpoint(dirpath=out_dir, save_last=True, save_top_k=0, every_n_train_steps=EVERY,
                                           every_n_epochs=0)]
    times = []
    step = model.training_step

    def timed(batch, i):
        t0 = time.perf_counter()
        step(batch, i)
        if variant == "blocking" and (i + 1) % EVERY == 0:
            torch.save({"state_dict": model.state_dict(),
                        "optimizer_states": [copy.deepcopy(o.state_dict()) for o in model.optimizers()]},
                       os.path.join(out_dir, "blocking.ckpt"))
        times.append(time.perf_counter() - t0)

    model.training_step = timed
    Trainer(max_epochs=1, max_steps=50).fit(model, MultiModalBatches(loaders, round_robin=True))  # warm-up: programs captured
    torch.cuda.synchronize()
    times.clear()
    trainer = Trainer(max_epochs=1, max_steps=STEPS, **kw)
    t0 = time.perf_counter()
    trainer.fit(model, MultiModalBatches(loaders, round_robin=True))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert len(times) == STEPS
    return 1e3 * sum(times) / STEPS, 1e3 * max(times), wall


def leg_loop(variants):
    print(f"{STEPS} steps of the C2 step through Trainer.fit (batch {BATCH}), a checkpoint every {EVERY} steps where one is "
          "taken; host time per step, wall time with the device drained and the last write finished:")
    labels = {"none": "no checkpoints                         ", "blocking": "blocking state_dict() + torch.save     ",
              "snapshot": "ModelCheckpoint on the snapshot path   "}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(2):
            for v in variants:
                mean, worst, wall = _loop(v, tmp)
                print(f"  {labels[v]}: mean {mean:7.3f} ms/step   max {worst:9.3f} ms   wall {wall:7.3f} s   (run {rep + 1})")
                sys.stdout.flush()


def leg_resources():
    csrc = os.path.join(ROOT, "mmvae_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    fields = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
              "Occupancy [waves/SIMD]")
    print("kernels of libmmvae_ckpt.so as hipcc --offload-arch=gfx950 -O3 reports them "
          "(VGPRs / AGPRs / scratch bytes per lane / VGPR spills / SGPR spills / LDS bytes / waves per SIMD):")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "ckpt_snapshot.hip"), "-o",
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
    ap.add_argument("--legs", default="entry,loop,resources")
    ap.add_argument("--variants", default="none,blocking,snapshot", help="of the loop leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        {"entry": leg_entry, "loop": lambda: leg_loop(args.variants.split(",")), "resources": leg_resources}[args.leg]()
        return 0
    lines = []
    for leg in args.legs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--variants", args.variants],
                               capture_output=True, text=True, timeout=LEGS[leg])
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
