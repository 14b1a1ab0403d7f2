#!/usr/bin/env python3
"""The C2 training loop fed from chunk files, with the feed's chunks gathered on the host (`--device-chunks 0`: the
loop of `bench.py --input npz`) or resident on the device (`--device-chunks 1`: one upload per chunk, one
`mmvae_csr_gather_rows_*` launch per batch).  Same data, same model, same loop either way: eight synthetic batches per
expert written as uncompressed npz-CSR / pkl chunks of four batches, read through SpeciesChunks ->
MultiModalBatches(round_robin) -> Prefetcher(depth 3) -> Lookahead -> training_step.  Prints ONE JSON line (ms/step,
cells/s).  For an A/B, alternate the two settings, one process per run, and compare medians.

`--normalize 1`: the chunk files hold the RAW counts behind the same batches and the feed normalises them on the way
(`SpeciesChunks(normalize="log1p_cpm")`: one launch per uploaded chunk with `--device-chunks 1`, one per batch without);
`--normalize 0` (default) reads pre-normalised files, as before."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--device-chunks", type=int, choices=[0, 1], default=0)
    ap.add_argument("--normalize", type=int, choices=[0, 1], default=0)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--config", default="c2", choices=["c2"])
    a = ap.parse_args()

    import pandas as pd
    import scipy.sparse as sp
    import torch

    import bench
    from mmvae_amd import data as mdata, synthetic
    from mmvae_amd.trainer import Lookahead, MultiModalBatches

    json_fd = os.dup(1)  # ONE JSON line on stdout: whatever native code prints goes to stderr
    os.dup2(2, 1)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    cfg = dict(synthetic.CONFIGS[a.config])
    B = cfg["batch"]
    model = bench.build_model(argparse.Namespace(config=a.config, genes="", hidden=0, no_engine=False), cfg, device).to(device)
    model.train()
    model.trainer.set_stage("training")
    model.optimizers()

    tmp = tempfile.mkdtemp(prefix="mmvae_bench_feed_")
    feeds = {}
    for i, (eid, G) in enumerate(cfg["experts"].items()):
        draw = synthetic.synthetic_raw_counts if a.normalize else synthetic.synthetic_counts
        rows = torch.cat([draw(B, G, seed=77 + 31 * i + j, device="cpu") for j in range(8)])
        meta = pd.concat([synthetic.synthetic_metadata(B, seed=9 + j) for j in range(8)], ignore_index=True)
        mdata.write_chunks(os.path.join(tmp, eid), eid, sp.csr_matrix(rows.numpy()), meta, chunk_rows=4 * B,
                           compressed=False)
        feeds[eid] = mdata.SpeciesChunks(os.path.join(tmp, eid), f"{eid}_train_counts_*.npz",
                                         f"{eid}_train_metadata_*.pkl", B, eid, seed=i, device=device,
                                         device_chunks=bool(a.device_chunks),
                                         **(dict(normalize="log1p_cpm") if a.normalize else {}))

    def endless():
        while True:
            yield from MultiModalBatches(feeds, seed=0, round_robin=True)

    steps = iter(Lookahead(mdata.Prefetcher(endless(), depth=3, device=device), model))
    n = 0

    def step():
        nonlocal n
        model.training_step(next(steps), n)
        n += 1

    # set-up (untimed): every expert's program is built on its first run and captured on its second; go on until a whole
    # round of steps has replayed its program
    period = len(cfg["experts"])
    for _ in range(16 * period):
        step()
    replayed = 0
    while replayed < 2 * period and n < 400:
        step()
        plan = getattr(model._engine, "last_plan", None) if model._engine else None
        replayed = replayed + 1 if (plan is None or (plan._graphs is not None and plan._runs >= 3)) else 0
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps):
        step()
        marks[i + 1].record()
    model._flush_engine()
    host_el = time.perf_counter() - t0
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    steps.close()  # stops the feed's threads before the interpreter shuts down
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps))
    loss = {k: float(v.detach()) for k, v in model.logged.items() if k.startswith("loss/")}
    out = {"metric": "cells/sec per MMVAE train step, npz-CSR chunks streamed from disk", "unit": "cells/s",
           "value": B * a.steps / el, "ms_per_step": el / a.steps * 1e3, "ms_per_step_median": per_step[len(per_step) // 2],
           "host_ms_per_step": host_el / a.steps * 1e3, "device_chunks": int(a.device_chunks), "normalize": int(a.normalize), "steps": a.steps,
           "warmup": a.warmup, "config": a.config, "batch": B, "path": "engine(hipGraph)" if model._engine else "module",
           "last_losses": loss, "device": torch.cuda.get_device_name(0)}
    os.write(json_fd, (json.dumps(out) + "\n").encode())
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
