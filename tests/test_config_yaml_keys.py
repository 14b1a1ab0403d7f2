"""The drop-in claim "model YAMLs in the reference's schema load unchanged" (YAML class paths) on this
repository's own files, with no reference checkout needed: every configs/model/*.yaml (class_path / init_args as the
reference's LightningCLI reads them, `cmmvae.*` class paths) is built through mmvae_amd.instantiate with `cmmvae.*`
resolved to this package, and the module must have the state_dict keys and shapes -- and the adversaries -- that the
REFERENCE's own classes build from the same file.  What the reference built is a fixture
(tests/golden/reference_checkpoint_keys.json: class name, keys, shapes, number of adversaries), recorded from a checkout
of the reference by tests/golden/make_reference_yaml.py.  Only the data-directory paths are substituted (labels_dir /
conditionals_directory point at a generated label tree), as in tests/test_reference_yaml.py, which checks the
reference's own YAMLs where a checkout of it is at hand.
Reference: configs/model/human_only.yaml:1-157, runners/cli.py:18-41, modules/cmmvae.py:18-49."""
import glob
import json
import os

import pytest
import yaml

from tests.test_reference_yaml import _conditions, _label_tree, _with_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "reference_checkpoint_keys.json")


def _model_yamls():
    return sorted(glob.glob(os.path.join(ROOT, "configs", "model", "*.yaml")))


def _recorded():
    with open(RECORD) as f:
        return json.load(f)


def test_every_model_yaml_has_what_the_reference_built_from_it():
    files = [os.path.relpath(p, ROOT) for p in _model_yamls()]
    assert "configs/model/c2_two_modality_20k.yaml" in files and sorted(_recorded()) == files
    assert any(r["n_adversarials"] > 0 for r in _recorded().values())


@pytest.mark.parametrize("path", _model_yamls(), ids=lambda p: os.path.relpath(p, ROOT))
def test_model_yaml_builds_the_reference_checkpoint_keys(path, tmp_path):
    from mmvae_amd import backend, instantiate
    from mmvae_amd.modules import base

    with open(path) as f:
        node = yaml.safe_load(f)
    node = _with_paths(node, _label_tree(str(tmp_path), _conditions(node)))
    ref_module = _recorded()[os.path.relpath(path, ROOT)]
    base.Adversarial.labels.clear()
    with backend.cpu_plumbing():
        model = instantiate.build(node)
        n_optimizers = len(model.configure_optimizers())
    assert type(model).__name__ == "CMMVAEModel" and type(model.module).__name__ == ref_module["module_class"]
    ours = {k: tuple(v.shape) for k, v in model.module.state_dict().items()}
    ref = {k: tuple(v) for k, v in ref_module["state_dict"].items()}
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref, [(k, ours[k], ref[k]) for k in ours if ours[k] != ref[k]][:5]
    assert all(k.startswith("module.") for k in model.state_dict())
    # the trainer-facing arguments of the file arrive where the reference puts them (cmmvae_model.py:40-57)
    args = node["init_args"]
    assert model.adv_weight == (args.get("adv_weight") or 1.0)
    # (`adversarials: null` leaves the attribute undefined in the reference, modules/cmmvae.py:46-49: recorded as 0; this
    # build accepts None as "no adversaries")
    assert len(model.module.adversarials) == ref_module["n_adversarials"]
    assert n_optimizers == len(model.module.experts) + 1 + len(model.module.adversarials)
    fn = args.get("kl_annealing_fn", {}).get("init_args", {})
    if "warmup_steps" in fn:  # `1e4` is a string to PyYAML: the schedule must still be numbers (annealing_fn.py:17-33)
        assert model.kl_annealing_fn.x == -float(fn["warmup_steps"]) and isinstance(model.kl_annealing_fn.m, float)
