#!/usr/bin/env python3
"""Golden vectors of models with LayerNorm in ordinary FCBlocks, produced by the REFERENCE's own modules the way
tests/golden/make_golden.py produces the others (its run_case drives the training steps; only the model builder differs:
make_golden's fixes use_layer_norm=False).  Runs only where the reference's sources are present:

    python tests/golden/make_golden_ln.py

ln_core:  the shared VAE's encoder of the reference's configs/model/configV3.yaml scaled down -- Linear -> LayerNorm(no
          affine) -> ReLU on all three layers, return_hidden [false, true, true] -- with one adversary on the first
          hidden representation, so that a gradient comes back into a LayerNorm layer's activation.
ln_mixed: LayerNorm without activation on the VAE decoder's first layer, BatchNorm + LayerNorm on a VAE encoder layer,
          LayerNorm with dropout and return_hidden (the adversaries' gradient bypasses the keep mask), LayerNorm on inner
          expert layers.
The fixtures hold data only (tests/ln_cases.py describes the layout of case["blocks"])."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT_DIR))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as MG  # noqa: E402
from tests import ln_cases  # noqa: E402


def blk(n, dropout=0.0, bn=False, ln=False, relu=True, return_hidden=False, **kw):
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n  # noqa: E731
    return dict(kw, dropout=per(dropout), bn=per(bn), ln=per(ln), relu=per(relu), return_hidden=per(return_hidden))


CASES = {
    "ln_core": dict(
        seed=83, experts={"human": 72, "mouse": 56}, Z=12, B=16, hidden_z=False, schedule=["human", "mouse", "human"],
        kl_weights=[1.0, 1.0, 0.5], adversarials=[[24, 16, 8]], conditions={"assay": 5, "sex": 2}, adv_weight=5,
        blocks=dict(expert_enc=blk(2, hidden=[48, 40], dropout=0.1, bn=True), expert_dec=blk(2, hidden=[40, 48]),
                    vae_enc=blk(3, layers=[40, 32, 24, 24], ln=True, return_hidden=[False, True, True]),
                    vae_dec=blk(3, layers=[12, 24, 32, 40]))),
    "ln_mixed": dict(
        seed=89, experts={"human": 72, "mouse": 56}, Z=12, B=20, hidden_z=True, schedule=["human", "mouse", "human"],
        kl_weights=[1.0, 0.5, 1.0], adversarials=[[32, 16, 8], [24, 8]], conditions={"assay": 5, "donor_id": 11},
        adv_weight=5,
        blocks=dict(expert_enc=blk(2, hidden=[48, 40], dropout=0.1, bn=[True, False], ln=[False, True]),
                    expert_dec=blk(2, hidden=[40, 48], ln=[True, False]),
                    vae_enc=blk(2, layers=[40, 32, 24], dropout=0.1, bn=[True, False], ln=True, return_hidden=True),
                    vae_dec=blk(2, layers=[12, 24, 40], ln=[True, False], relu=[False, True]))),
}


def build_reference(case, tmpdir):
    """make_golden.build_reference for a case of tests/ln_cases.py."""
    import cmmvae.modules as modules
    from cmmvae.modules.base.init import he_init_weights

    module = ln_cases.build_modules(case, tmpdir, modules)
    torch.manual_seed(case["seed"])
    he_init_weights(module)
    g = torch.Generator().manual_seed(case["seed"] + 1)
    for name, p in module.named_parameters():
        if name.endswith("bias") or name.endswith("bn.weight"):
            with torch.no_grad():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    drops = {}
    for name, m in list(module.named_modules()):
        for cname, child in list(m.named_children()):
            if isinstance(child, nn.Dropout):
                ed = MG.ExplicitDropout(child.p)
                setattr(m, cname, ed)
                drops[f"{name}.{cname}"] = ed
    return module, drops


def main():
    if not os.path.isdir(MG.REF_SRC):
        print(f"{MG.REF_SRC} not present: golden vectors can only be generated in the build container; nothing done.")
        return 0
    sys.path.insert(0, MG.REF_SRC)
    MG.build_reference = build_reference
    torch.set_num_threads(1)
    for name, case in CASES.items():
        out = MG.run_case(dict(case))
        path = os.path.join(OUT_DIR, f"{name}.npz")
        if os.path.exists(path):  # regenerated vectors must reproduce the committed ones bit for bit
            old = np.load(path)
            for k in old.files:
                assert k in out and np.array_equal(np.asarray(old[k]), np.asarray(out[k])), f"{name}: {k} changed"
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
