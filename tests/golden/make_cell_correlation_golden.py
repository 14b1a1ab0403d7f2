"""Writes tests/golden/cell_correlation.npz: two small (cis ; cross) pairs per species and the eight numbers the
reference's own calc_correlations (runners/run_correlations.py:18-60) returns for them.

Runs only where the reference checkout is present:  python tests/golden/make_cell_correlation_golden.py /path/to/reference
The reference function is loaded by FILE PATH (the `runners` package itself imports plotting and embedding libraries
that the function does not need).  The fixture holds numbers only.

Inputs: ReLU-like values (many exact zeros, as behind an output ReLU), a shared component so that the cross block
correlates with the cis block, one all-zero row in each matrix.  Both stacked matrices of a case are cut at the same
row count, because the reference slices both at the human sample count."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"split_7_5x70": (7, 5, 70), "split_6_6x61": (6, 6, 61)}  # name -> (cis rows, cross rows, genes)
COLUMNS = ("human_cis", "human_cross", "human_comb", "human_rel", "mouse_cis", "mouse_cross", "mouse_comb", "mouse_rel")


def stacked(rng, n, m, G, zero_row):
    shared = rng.standard_normal(G)
    x = np.maximum(rng.standard_normal((n + m, G)) + 0.8 * shared - 0.4, 0.0)
    x[n:] = np.maximum(x[n:] + 0.5 * rng.standard_normal((m, G)), 0.0)
    x[zero_row] = 0.0
    return x.astype(np.float32)


def main(reference_root: str) -> None:
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, os.path.join(reference_root, "src"))
    path = os.path.join(reference_root, "src", "cmmvae", "runners", "run_correlations.py")
    spec = importlib.util.spec_from_file_location("reference_run_correlations", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    rng = np.random.default_rng(20240607)
    for name, (n, m, G) in CASES.items():
        human = stacked(rng, n, m, G, zero_row=1)
        mouse = stacked(rng, n, m, G, zero_row=n + 2)
        table = mod.calc_correlations(human.astype(np.float64), mouse.astype(np.float64), n)
        out[f"{name}/human"], out[f"{name}/mouse"] = human, mouse
        out[f"{name}/n"] = np.int64(n)
        out[f"{name}/expected"] = np.array([float(table[c].iloc[0]) for c in COLUMNS], dtype=np.float64)
        print(name, dict(zip(COLUMNS, out[f"{name}/expected"])))
    np.savez(os.path.join(HERE, "cell_correlation.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
