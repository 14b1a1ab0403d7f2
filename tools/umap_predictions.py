#!/usr/bin/env python3
"""Plot UMAP embeddings coloured by metadata categories: the reference's `umap_predictions` command
(runners/umap_predictions.py:318-356) with its option names, on the device (mmvae_amd.plots.generate_umap).

    python tools/umap_predictions.py --directory run/predictions.h5 --categories cell_type --categories tissue --keys z

--directory is a directory holding {key}_embeddings.npz / {key}_metadata.pkl (or the stored {key}_umap_* pair), or a
predictions.h5.  --categories and --keys may be given several times, as with click's multiple=True.  Prints the paths
of the images it wrote, one per line.  TensorBoard logging is not part of this tool.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Plot UMAP embeddings coloured by metadata categories.")
    ap.add_argument("--directory", default=os.environ.get("DIRECTORY") or None, required=not os.environ.get("DIRECTORY"),
                    help="Directory where embeddings and metadata are stored, or a predictions.h5.")
    ap.add_argument("--categories", action="append", required=True, help="Categories to color by (repeatable).")
    ap.add_argument("--keys", action="append", required=True,
                    help="Keys that prefix the embeddings and metadata (repeatable).")
    ap.add_argument("--save_dir", default=None, help="Directory to store PNGs")
    ap.add_argument("--method", default="", help="Method name to add to graph title")
    args = ap.parse_args(argv)
    if not os.path.exists(args.directory):
        ap.error(f"--directory: {args.directory} does not exist")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    from mmvae_amd.plots import generate_umap

    for path in generate_umap(args.directory, tuple(args.categories), tuple(args.keys), method=args.method or "",
                              save_dir=args.save_dir):
        print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
