#!/usr/bin/env python3
"""What a per-step learning-rate schedule costs the C2 training loop.

Resident synthetic batches, bench.py's model and loop (round-robin over the experts, one batch of look-ahead), steps
timed between device synchronises.  One call alternates blocks of `--steps` steps: constant lr, then lr rewritten before
every step through `param_groups` (what a torch.optim.lr_scheduler or the model's lr_schedule_fn does), `--rounds` times.
Two constant blocks per round give the A/A spread the scheduled blocks are held against.  The tool writes
`param_groups` itself and uses nothing newer, so the same file measures a commit whose engine re-captures its programs
on every change of lr (give it a short `--steps` then).  Prints ONE JSON line."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=["c2"])
    a = ap.parse_args()

    import torch

    import bench
    from mmvae_amd import synthetic

    json_fd = os.dup(1)  # ONE JSON line on stdout: whatever native code prints goes to stderr
    os.dup2(2, 1)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    cfg = dict(synthetic.CONFIGS[a.config])
    B = cfg["batch"]
    model = bench.build_model(argparse.Namespace(config=a.config, genes="", hidden=0, no_engine=False), cfg, device).to(device)
    model.train()
    model.trainer.set_stage("training")
    optimizers = model.optimizers()
    base = [o.param_groups[0]["lr"] for o in optimizers]
    eids = list(cfg["experts"].keys())
    data = {eid: [(synthetic.synthetic_counts(B, G, seed=1234 + 97 * i + 13 * j, device=device),
                   synthetic.synthetic_metadata(B, seed=5 + j)) for j in range(2)]
            for i, (eid, G) in enumerate(cfg["experts"].items())}

    def batch_of(i):
        eid = eids[i % len(eids)]
        x, meta = data[eid][(i // len(eids)) % 2]
        return x, meta, eid

    n = 0

    def step(scheduled: bool):
        nonlocal n
        # a cosine between 0.5 and 1 of the base lr with a period of 64 steps: another value on every step
        f = 0.75 + 0.25 * math.cos(2 * math.pi * n / 64) if scheduled else 1.0
        for o, lr in zip(optimizers, base):
            o.param_groups[0]["lr"] = lr * f
        model.hint_next_batch(batch_of(n + 1))
        model.training_step(batch_of(n), n)
        n += 1

    def block(scheduled: bool, steps: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(scheduled)
        model._flush_engine()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for _ in range(16 * len(eids)):  # set-up (untimed): every program built, captured and replayed
        step(False)
    block(False, a.warmup)
    block(True, min(a.warmup, a.steps))
    const_a, const_b, sched = [], [], []
    for _ in range(a.rounds):
        const_a.append(block(False, a.steps))
        sched.append(block(True, a.steps))
        const_b.append(block(False, a.steps))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    engine = model._engine
    out = {"metric": "ms per C2 training step, constant lr against lr rewritten before every step", "unit": "ms/step",
           "constant_ms": med(const_a + const_b), "scheduled_ms": med(sched),
           "constant_blocks_ms": [round(v, 4) for pair in zip(const_a, const_b) for v in pair],
           "scheduled_blocks_ms": [round(v, 4) for v in sched],
           "aa_spread_ms": max(const_a + const_b) - min(const_a + const_b),
           "scheduled_minus_constant_ms": med(sched) - med(const_a + const_b),
           "plans": len(engine._plans) if engine else 0,
           "settings_rebuilds": getattr(engine, "_sig_changes", None) if engine else None,
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "config": a.config, "batch": B,
           "path": "engine(hipGraph)" if engine else "module", "device": torch.cuda.get_device_name(0)}
    os.write(json_fd, (json.dumps(out) + "\n").encode())


if __name__ == "__main__":
    main()
