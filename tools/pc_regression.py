#!/usr/bin/env python3
"""Principal-component regression of stored latent embeddings, on the device (mmvae_amd.pca.pc_regression).

    python tools/pc_regression.py --directory run/predictions.h5 --keys z --covariates species --covariates total_counts

--directory is a directory holding {key}_embeddings.npz / {key}_metadata.pkl, or a predictions.h5 -- the two input forms
of tools/graph_metrics.py, through the same loaders.  --keys and --covariates may be given several times; a numeric
metadata column is regressed as it is, any other as a categorical one.  Writes pcr.{key}.csv (one row per covariate: its
kind, classes, cells, components and the variance-weighted R2) and pcr.{key}.components.csv (the explained variance ratio
and R2 of every component) into --save_dir (default: next to the input), and prints the paths, one per line.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Principal-component regression of latent embeddings.")
    ap.add_argument("--directory", default=os.environ.get("DIRECTORY") or None, required=not os.environ.get("DIRECTORY"),
                    help="Directory where embeddings and metadata are stored, or a predictions.h5.")
    ap.add_argument("--keys", action="append", required=True,
                    help="Keys that prefix the embeddings and metadata (repeatable).")
    ap.add_argument("--covariates", action="append", default=None,
                    help="Metadata columns to regress on the components (repeatable; default: species).")
    ap.add_argument("--n_comps", type=int, default=None, help="Components kept (default: all)")
    ap.add_argument("--save_dir", default=None, help="Directory to store the tables")
    args = ap.parse_args(argv)
    if not os.path.exists(args.directory):
        ap.error(f"--directory: {args.directory} does not exist")
    args.covariates = args.covariates or ["species"]
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    from mmvae_amd.pca import pcr_from_predictions

    for path in pcr_from_predictions(args.directory, tuple(args.keys), tuple(args.covariates), save_dir=args.save_dir,
                                     n_comps=args.n_comps):
        print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
