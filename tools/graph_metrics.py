#!/usr/bin/env python3
"""Graph connectivity and kBET of stored latent embeddings, on the device (mmvae_amd.graph_metrics.graph_metrics).

    python tools/graph_metrics.py --directory run/predictions.h5 --keys z --batch species --labels cell_type

--directory is a directory holding {key}_embeddings.npz / {key}_metadata.pkl, or a predictions.h5 -- the two input forms
of tools/integration_metrics.py, through the same loaders.  --keys and --labels may be given several times.  Writes
graph_metrics.{key}.csv (one row per label column: graph connectivity, components, rounds, the whole-graph kBET rejection
rate and the per-label kBET score) and graph_metrics.{key}.{label}.csv (one row per class) into --save_dir (default:
next to the input), and prints the paths, one per line.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Graph connectivity and kBET of latent embeddings.")
    ap.add_argument("--directory", default=os.environ.get("DIRECTORY") or None, required=not os.environ.get("DIRECTORY"),
                    help="Directory where embeddings and metadata are stored, or a predictions.h5.")
    ap.add_argument("--keys", action="append", required=True,
                    help="Keys that prefix the embeddings and metadata (repeatable).")
    ap.add_argument("--batch", default="species", help="Metadata column of the batches to be mixed")
    ap.add_argument("--labels", action="append", default=None,
                    help="Metadata columns of the labels to be kept (repeatable; default: cell_type).")
    ap.add_argument("--save_dir", default=None, help="Directory to store the tables")
    ap.add_argument("--n_neighbors", type=int, default=15, help="Neighbours of the kNN graph, the point included (<= 64)")
    ap.add_argument("--alpha", type=float, default=0.05, help="Significance level of the kBET rejections")
    args = ap.parse_args(argv)
    if not os.path.exists(args.directory):
        ap.error(f"--directory: {args.directory} does not exist")
    args.labels = args.labels or ["cell_type"]
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    from mmvae_amd.graph_metrics import metrics_from_predictions

    for path in metrics_from_predictions(args.directory, tuple(args.keys), args.batch, tuple(args.labels),
                                         save_dir=args.save_dir, n_neighbors=args.n_neighbors, alpha=args.alpha):
        print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
