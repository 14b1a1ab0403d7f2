#!/usr/bin/env python3
"""Record the fixture of tests/test_config_yaml_keys.py from a checkout of the reference (zdebruine/MMVAE):

    python tests/golden/make_reference_yaml.py PATH_TO_REFERENCE_CHECKOUT

Every model YAML of this repository (configs/model/*.yaml, written in the reference's LightningCLI schema) is built with
the REFERENCE's own classes, imported from <reference>/src (its `cmmvae.models` needs Lightning and is not importable,
so the reference side is the `module:` subtree), through the same class_path / init_args builder and with the same
data-directory substitution as the test; arguments this build adds to the schema (EXTENSIONS: they hold no parameters)
are left out of what the reference builds.  Recorded per file: the module's class name, its state_dict keys and shapes and
its number of adversaries.  Written to tests/golden/reference_checkpoint_keys.json (names and shapes only)."""
import glob
import json
import os
import sys
import tempfile

import torch
import yaml

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_reference_yaml as T  # noqa: E402  (the label tree and path substitution of both YAML tests)

EXTENSIONS = ("n_samples",)  # Encoder(n_samples=K): the K-sample log-mean-exp ELBO of configs C3 / C5


def build_reference_module(ref, node):
    """The `module:` subtree with the REFERENCE's classes, through the same class_path / init_args builder."""
    from mmvae_amd import instantiate

    src = os.path.join(ref, "src")
    if src not in sys.path:
        sys.path.insert(0, src)
    import cmmvae.modules.base.components as ref_components  # noqa: F401  (torch + pandas only: importable here)

    ref_components.Adversarial.labels.clear() if hasattr(ref_components.Adversarial, "labels") else None
    aliases, instantiate.ALIASES = instantiate.ALIASES, {}
    try:
        return instantiate.build(node["init_args"]["module"])
    finally:
        instantiate.ALIASES = aliases


def main(ref):
    record = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "model", "*.yaml"))):
        with open(path) as f:
            node = yaml.safe_load(f)
        T._walk(node, lambda parent, k, v: parent.pop(k) if k in EXTENSIONS else None)
        with tempfile.TemporaryDirectory() as tmp:
            node = T._with_paths(node, T._label_tree(tmp, T._conditions(node)))
            torch.manual_seed(0)
            module = build_reference_module(ref, node)
        try:
            n_adv = len(module.adversarials)
        except AttributeError:  # `adversarials: null` leaves the attribute undefined in the reference
            n_adv = 0
        record[os.path.relpath(path, ROOT)] = {
            "module_class": type(module).__name__, "n_adversarials": n_adv,
            "state_dict": {k: list(v.shape) for k, v in module.state_dict().items()}}
    with open(os.path.join(GOLDEN, "reference_checkpoint_keys.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(record)} model files recorded")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
