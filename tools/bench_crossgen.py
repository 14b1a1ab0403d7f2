#!/usr/bin/env python3
"""Cross-generation and the statistics computed on it, measured.

Five legs, each in a child process of its own under its own time limit (a leg that faults, aborts or runs out of time
ends the run: nothing more is started on the device):

  step-c2    ms per CMMVAEModel.cross_generate_step to ALL experts, captured engine against the module path, interleaved
             blocks on one device: C2's model (2 experts, 20 000 genes, B = 512)
  step-full  the same at the reference's gene counts (60 530 / 52 437, B = 512)
  pearson    us of mmvae_col_pearson_f32 at (100, 60 530), (512, 20 000), (512, 60 530) with the achieved GB/s against
             the bytes of both matrices, and us of the torch statement of the same statistic (centre, multiply, sum; no
             torch.corrcoef) on the same inputs
  cellcorr   us of mmvae_stats_row_corr_f32 (cell-by-cell correlation of a cis on a cross generation and its block
             means) at (100 + 100, 20 000), (100 + 100, 60 530), (512 + 512, 20 000), and of torch.corrcoef on the device
             in fp32 and in fp64 on the stacked copy, the copy's time listed separately
  metadisc   ms per MetaDiscriminators.step (cross-generation, the latent discriminator and the other expert's
             discriminator: GEMM, fused tail kernel, GEMM, fused Adam each) at C2 and at the reference's gene counts,
             B = 512, against the same step done with nn.Sequential + torch.optim.Adam on the device, interleaved blocks;
             and us of one train_step of the gene-wide discriminator alone against its stock-torch counterpart

Nothing is asserted: the numbers are reported.  Output: the lines below, also written to --out (default
profiles/crossgen.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENES = {"c2": {"human": 20000, "mouse": 20000}, "full": {"human": 60530, "mouse": 52437}}
PEARSON_SHAPES = [(100, 60530), (512, 20000), (512, 60530)]
CELLCORR_SHAPES = [(100, 100, 20000), (100, 100, 60530), (512, 512, 20000)]
LEGS = {"step-c2": 240, "step-full": 300, "pearson": 240, "cellcorr": 240, "metadisc": 420}  # seconds


def leg_step(which: str, blocks: int, steps: int):
    import pandas as pd
    import torch

    from mmvae_amd import synthetic

    B, genes = 512, GENES[which]
    model = synthetic.build_model(genes, use_engine=True, seed=0).cuda()
    model.eval()
    model.trainer.set_stage("prediction")
    xs = {e: synthetic.synthetic_counts(B, G, seed=7 + i, device="cuda") for i, (e, G) in enumerate(genes.items())}
    eids = list(genes)
    frames = {e: pd.DataFrame({"cell": range(B)}) for e in eids}  # (built once: no host allocation inside the timed blocks)

    def block(engine: bool, n: int) -> float:
        model.use_engine = engine
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            e = eids[i % len(eids)]
            model.cross_generate_step((xs[e], frames[e], e))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for engine in (True, False):  # every program built, captured and replayed; every code object loaded
        block(engine, 8 * len(eids))
    assert model._engine and all(k[0] == "generate" for k in model._engine._plans)
    eng, mod = [], []
    for _ in range(blocks):
        eng.append(block(True, steps))
        mod.append(block(False, steps))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print(f"cross_generate_step to all experts, {which} ({'/'.join(str(g) for g in genes.values())} genes, B = {B}), "
          f"{blocks} interleaved blocks of {steps} calls, clones returned:")
    print(f"  captured engine : {med(eng):8.3f} ms / call   (blocks {' '.join(f'{v:.3f}' for v in eng)})")
    print(f"  module path     : {med(mod):8.3f} ms / call   (blocks {' '.join(f'{v:.3f}' for v in mod)})")
    print(f"  module / engine : {med(mod) / med(eng):8.2f} x")


def timed(fn, n):
    import torch

    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def leg_pearson(reps: int):
    import torch

    from mmvae_amd import ops, synthetic

    def torch_statement(a, b):
        da, db = a - a.mean(0), b - b.mean(0)
        return (da * db).sum(0) / torch.sqrt((da * da).sum(0) * (db * db).sum(0))

    print(f"per-gene Pearson correlation, {reps} back-to-back calls each (device events; two launches per HIP call); "
          "GB/s = bytes of both matrices / time:")
    for B, G in PEARSON_SHAPES:
        ld = (G + 3) // 4 * 4  # rows as the engine's xhat buffers hold them: 16-byte regular
        a = torch.zeros(B, ld, device="cuda")[:, :G]
        b = torch.zeros(B, ld, device="cuda")[:, :G]
        a.copy_(synthetic.synthetic_counts(B, G, seed=3, device="cuda"))
        b.copy_(a + 0.25 * torch.randn(B, G, device="cuda"))
        ac, bc = a.contiguous(), b.contiguous()
        out = torch.empty(G, device="cuda")
        nbytes = 2 * B * G * 4
        rows = [("mmvae_col_pearson_f32, padded rows (16-byte loads)", timed(lambda: ops.col_pearson(a, b, out=out), reps))]
        if G % 4:
            rows.append(("mmvae_col_pearson_f32, contiguous (element-wise)", timed(lambda: ops.col_pearson(ac, bc, out=out), reps)))
        rows.append(("torch: centre, multiply, sum (fp32)", timed(lambda: torch_statement(ac, bc), max(reps // 4, 5))))
        r, want = ops.col_pearson(a, b), torch_statement(ac.double(), bc.double())
        live = ~torch.isnan(r)
        err = float((r[live].double() - want[live]).abs().max())
        print(f"  ({B}, {G}): {int((~live).sum())} constant genes, max |r - fp64 torch| {err:.2e}")
        for name, us in rows:
            print(f"    {name:<52s} {us:9.1f} us   {nbytes / us / 1e3:8.1f} GB/s")


def leg_cellcorr(reps: int):
    import torch

    from mmvae_amd import ops, synthetic

    print(f"cell-by-cell correlation of (cis ; cross), {reps} back-to-back calls each (device events; four launches per "
          "HIP call); GFLOP/s = 2 R^2 G / time (the full square: the kernel computes one triangle):")
    for n_a, n_b, G in CELLCORR_SHAPES:
        R, ld = n_a + n_b, (G + 3) // 4 * 4  # rows as the engine's xhat buffers hold them: 16-byte regular
        a = torch.zeros(n_a, ld, device="cuda")[:, :G]
        b = torch.zeros(n_b, ld, device="cuda")[:, :G]
        a.copy_(synthetic.synthetic_counts(n_a, G, seed=3, device="cuda"))
        b.copy_(torch.relu(synthetic.synthetic_counts(n_b, G, seed=4, device="cuda") + 0.25 * torch.randn(n_b, G, device="cuda")))
        ac, bc = a.contiguous(), b.contiguous()
        out = torch.empty(R, R, device="cuda")
        stacked = torch.cat([ac, bc], 0)
        stacked64 = stacked.double()
        rows = [("mmvae_stats_row_corr_f32, padded rows (16-byte loads)", timed(lambda: ops.row_corrcoef(a, b, out=out), reps)),
                ("mmvae_stats_row_corr_f32, block means only (no matrix)", timed(lambda: ops.row_corrcoef(a, b, want_matrix=False), reps))]
        if G % 4:
            rows.append(("mmvae_stats_row_corr_f32, contiguous (element-wise)", timed(lambda: ops.row_corrcoef(ac, bc, out=out), reps)))
        slow = max(reps // 10, 5)
        rows.append(("torch.cat of the two operands (the stacked copy)", timed(lambda: torch.cat([ac, bc], 0), reps)))
        rows.append(("torch.corrcoef, fp32, on the stacked copy", timed(lambda: torch.corrcoef(stacked), slow)))
        rows.append(("torch.corrcoef, fp64, on the stacked copy", timed(lambda: torch.corrcoef(stacked64), slow)))
        corr, stats = ops.row_corrcoef(a, b)
        want = torch.corrcoef(stacked64)
        live = ~torch.isnan(want)
        err = float((corr.double()[live] - want[live]).abs().max())
        err32 = float((torch.corrcoef(stacked).double()[live] - want[live]).abs().max())
        s = stats.cpu().numpy()
        print(f"  ({n_a} + {n_b}, {G}): {int(s[4] + s[5])} constant rows, cis {s[0]:.6f} cross {s[1]:.6f} comb {s[2]:.6f} "
              f"rel {s[3]:.6f}; max |corr - fp64 torch.corrcoef| {err:.2e} (fp32 torch.corrcoef: {err32:.2e})")
        for name, us in rows:
            print(f"    {name:<56s} {us:9.1f} us   {2.0 * R * R * G / us / 1e3:9.1f} GFLOP/s")


def leg_metadisc(blocks: int, steps: int, reps: int):
    import pandas as pd
    import torch
    import torch.nn.functional as F

    from mmvae_amd import synthetic
    from mmvae_amd.modules.meta_discriminator import MetaDiscriminators

    B = 512
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for which, genes in GENES.items():
        model = synthetic.build_model(genes, use_engine=True, seed=0).cuda()
        model.eval()
        model.trainer.set_stage("prediction")
        eids = list(genes)
        xs = {e: synthetic.synthetic_counts(B, G, seed=7 + i, device="cuda") for i, (e, G) in enumerate(genes.items())}
        frames = {e: pd.DataFrame({"cell": range(B)}) for e in eids}
        torch.manual_seed(0)
        mds = MetaDiscriminators(model)
        stock = {k: d.as_sequential().cuda() for k, d in mds.discriminators.items()}
        sopt = {k: torch.optim.Adam(v.parameters(), lr=1e-3) for k, v in stock.items()}
        truth = {e: torch.full((B, 1), mds.labels[e], device="cuda") for e in eids}

        def stock_train(name, matrix, y):
            sopt[name].zero_grad(set_to_none=True)
            with torch.enable_grad():
                loss = F.binary_cross_entropy(stock[name](matrix), y, reduction="mean")
                loss.backward()
            sopt[name].step()
            return loss

        def stock_step(e):
            others = [t for t in eids if t != e]
            out = model.cross_generate_step((xs[e], frames[e], e), targets=others)
            stock_train("latent", out["z"][0], truth[e])
            for t in others:
                stock_train(t, out[f"xhat_{t}"][0], truth[e])

        def block(ours: bool, n: int) -> float:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                e = eids[i % len(eids)]
                if ours:
                    mds.step((xs[e], frames[e], e))
                else:
                    stock_step(e)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for ours in (True, False):
            block(ours, 8 * len(eids))
        a, b = [], []
        for _ in range(blocks):
            a.append(block(True, steps))
            b.append(block(False, steps))
        print(f"MetaDiscriminators.step, {which} ({'/'.join(str(g) for g in genes.values())} genes, B = {B}, hidden 128/64), "
              f"{blocks} interleaved blocks of {steps} steps:")
        print(f"  HIP (GEMM + fused tail + GEMM + fused Adam) : {med(a):8.3f} ms / step   (blocks {' '.join(f'{v:.3f}' for v in a)})")
        print(f"  nn.Sequential + torch.optim.Adam            : {med(b):8.3f} ms / step   (blocks {' '.join(f'{v:.3f}' for v in b)})")
        print(f"  stock / HIP                                 : {med(b) / med(a):8.2f} x")
        t = eids[1]
        xhat = model.cross_generate_step((xs[eids[0]], frames[eids[0]], eids[0]), targets=[t])[f"xhat_{t}"][0]
        us_hip = timed(lambda: mds[t].train_step(xhat, 0.0), reps)
        us_stock = timed(lambda: stock_train(t, xhat, truth[eids[0]]), reps)
        us_lat = timed(lambda: mds["latent"].train_step(xs[eids[0]][:, :mds["latent"].in_features].contiguous(), 0.0), reps)
        print(f"  one train_step of the {genes[t]}-wide discriminator alone, {reps} back-to-back calls: HIP {us_hip:9.1f} us, "
              f"stock torch {us_stock:9.1f} us ({us_stock / us_hip:.2f} x); the latent discriminator: HIP {us_lat:9.1f} us")
        del model, mds, stock, sopt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=list(LEGS), help="run ONE leg in this process (what the driver starts)")
    ap.add_argument("--legs", default=",".join(LEGS), help="driver: the legs to run, in order")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossgen.txt"))
    a = ap.parse_args()
    if a.leg:
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_crossgen: no GPU -- a measurement path does not fall back")
        print(f"# {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}, torch {torch.__version__}")
        if a.leg == "pearson":
            leg_pearson(a.reps)
        elif a.leg == "cellcorr":
            leg_cellcorr(a.reps)
        elif a.leg == "metadisc":
            leg_metadisc(a.blocks, a.steps, a.reps)
        else:
            leg_step(a.leg.split("-")[1], a.blocks, a.steps)
        return
    lines = []
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--blocks", str(a.blocks), "--steps", str(a.steps),
               "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=LEGS[leg])
        except subprocess.TimeoutExpired:
            lines.append(f"[{leg}] not measured: no result within {LEGS[leg]} s; the run ends here")
            break
        if p.returncode != 0:
            lines.append(f"[{leg}] not measured: exit code {p.returncode}; the run ends here\n{p.stderr[-2000:]}")
            break
        lines.append(f"[{leg}]\n{p.stdout.rstrip()}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
