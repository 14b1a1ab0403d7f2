#!/usr/bin/env python3
"""Raw census chunks -> normalised chunks, the reference's normalisation pass
(scripts/data-preprocessing/: normalize_data per chunk, census_data_stats.py's per-file table) without its per-row loop.

  python tools/normalize_chunks.py --directory D --species NAME --out OUT [--target-sum 1e4] [--device cuda|cpu]

For every NAME*.npz / NAME*.pkl pair of D, in file-number order: the chunk is uploaded, normalised by one launch of
mmvae_prep_csr_log1p_norm_* (mmvae_amd.preprocess.normalize_csr_; numpy with --device cpu) and downloaded; the
normalised npz is written under OUT with the same name and the metadata pickle is copied unchanged.
OUT/NAME_data_distribution.csv gets one `file, mean, std` row per chunk: mean and population standard deviation of the
RAW per-cell totals, from the row sums the kernel produced on the way (the reference's get_data_stats)."""
import argparse
import csv
import glob
import os
import re
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def file_number(path: str) -> int:
    m = re.search(r"_(\d+)", os.path.basename(path))
    return int(m.group(1)) if m else 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--directory", required=True)
    ap.add_argument("--species", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--target-sum", type=float, default=1e4)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    a = ap.parse_args(argv)

    import numpy as np
    import scipy.sparse as sp
    import torch

    from mmvae_amd.preprocess import RowSumStats, normalize_csr_

    npz = sorted(glob.glob(os.path.join(a.directory, f"{a.species}*.npz")), key=file_number)
    pkl = sorted(glob.glob(os.path.join(a.directory, f"{a.species}*.pkl")), key=file_number)
    if not npz or len(npz) != len(pkl):
        print(f"{a.directory}: {len(npz)} npz and {len(pkl)} pkl files match {a.species}*", file=sys.stderr)
        return 1
    if os.path.abspath(a.out) == os.path.abspath(a.directory):
        print("--out must not be the input directory: the raw chunks would be overwritten", file=sys.stderr)
        return 1
    os.makedirs(a.out, exist_ok=True)
    rows, total = [], RowSumStats()
    for data_path, meta_path in zip(npz, pkl):
        m = sp.load_npz(data_path).tocsr()
        if m.shape[0] == 0:
            print(f"{data_path}: no rows", file=sys.stderr)
            return 1
        # a chunk of 2^31 stored elements or more keeps int64 row pointers
        idx = torch.int32 if m.nnz <= 0x7fffffff and m.shape[1] <= 0x7fffffff else torch.int64
        crow = torch.from_numpy(m.indptr.astype(np.int64)).to(idx)
        col = torch.from_numpy(m.indices.astype(np.int64)).to(idx)
        val = torch.from_numpy(m.data.astype(np.float32))  # (a copy: the loaded matrix is left alone)
        csr = torch.sparse_csr_tensor(crow.to(a.device), col.to(a.device), val.to(a.device), size=m.shape)
        csr, sums = normalize_csr_(csr, target_sum=a.target_sum, return_row_sums=True)
        one = RowSumStats.of(sums)
        total.update(sums)
        out = sp.csr_matrix((csr.values().cpu().numpy(), m.indices, m.indptr), shape=m.shape)
        sp.save_npz(os.path.join(a.out, os.path.basename(data_path)), out)
        shutil.copyfile(meta_path, os.path.join(a.out, os.path.basename(meta_path)))
        rows.append((os.path.basename(data_path), one.mean, one.std))
        print(f"{os.path.basename(data_path)}: {m.shape[0]} cells, {m.nnz} stored, mean {one.mean:.6g} std {one.std:.6g}")
    with open(os.path.join(a.out, f"{a.species}_data_distribution.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["file", "mean", "std"])
        w.writerows(rows)
    print(f"all {total.n} cells: mean {total.mean:.6g} std {total.std:.6g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
