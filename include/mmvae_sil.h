/*
 * mmvae_sil.h -- C-ABI of libmmvae_sil.so: silhouette widths of latent embeddings, on the MI355X (gfx950).
 *
 * The kNN-graph metrics of mmvae_mix.h are local: they see a cell's 63 nearest neighbours.  The silhouette is their
 * global companion (the ASW of the scIB benchmark, Luecken et al. 2022): for every cell, the mean distance to the cells
 * of its own class against the mean distance to the nearest other class, over ALL cells.  That is one O(N^2 D) pass; it
 * walks the exact-fp32 MFMA Gram tiles of the kNN pass (mmvae_umap.h) and keeps per-class sums instead of a top-k, so the
 * N x N matrix never exists.  A library and a version counter of its own, so that it moves neither the training step's
 * ABI nor the UMAP library's.
 *
 * Conventions are those of mmvae_umap.h and mmvae_mix.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as
 * void*.  Calls only enqueue work: no allocation, no host synchronisation, no hidden state.  Shapes are validated on the
 * host BEFORE anything is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.  No atomics: two calls on
 * the same inputs give the same bits.
 *
 * Input.  x [N, D] fp32, row i at x + i ldx, ldx >= D, 1 <= D <= MMVAE_SIL_MAX_D, N >= 1; the columns of a row past D are
 * never read.  The caller has sorted the rows so that the cells of one class are contiguous -- such a range is a RUN --
 * and the runs of one GROUP are adjacent:
 *
 *     run_ptr [R + 1] int32    run boundaries: run_ptr[0] = 0, strictly increasing, run_ptr[R] = N
 *     run_group [R] int32      the group of every run, non-decreasing
 *     1 <= R <= N
 *
 * The contents of both arrays are trusted (as idx is in mmvae_mix.h).  A silhouette is taken inside a group: pairs of
 * different groups are never compared, and a workgroup walks only the columns of the groups its rows lie in, so the pass
 * costs sum_g n_g^2 pairs.  One group = the silhouette of the classes over all cells (label ASW); class = batch and group =
 * cell type = the batch silhouette inside every cell type (batch ASW).
 *
 * Distance d(i, j), by `metric`:
 *
 *   0  Euclidean   d = sqrt(max(0, n_i + n_j - 2 g_ij)), g_ij the exact-fp32 inner product of rows i and j (one fmaf chain
 *                  over D, as the fp32 MFMA computes it) and n_i = g_ii by that same chain: two bit-equal rows have
 *                  n_i = n_j = g_ij and therefore distance exactly 0.  (Nothing is clamped to 0 by a threshold.)  The
 *                  Gram form cancels when the rows are far from the origin: the caller centres them first.
 *   1  cosine      d = max(0, 1 - <u_i, u_j>), u the unit rows of mmvae_umap_knn_cosine_f32: x_i / |x_i| with the norm
 *                  from an fp64 sum of squares; a zero row is the zero vector.
 *
 * Per row i, in run r (n_r rows) of group g:
 *
 *   a_i       = sum over j in r, j != i, of d(i, j), / (n_r - 1);  0 when n_r = 1
 *   m_r'      = sum over j in r' of d(i, j), / n_r'                for every other run r' of group g
 *   b_i       = min over r' of m_r';   nearest_i = the r' that attains it, ties going to the smaller index
 *   s_i       = 0 when n_r = 1 or max(a_i, b_i) = 0 (scikit-learn's conventions), else (b_i - a_i) / max(a_i, b_i)
 *
 * and b_i = NaN, nearest_i = -1, s_i = NaN where the group has no other run.  Pair distances are fp32; a sum over a run
 * is fp64 across the column tiles (the at most 64 columns of one tile are summed in fp32, in a fixed order); the
 * divisions and s are fp64.  Outputs a, b, s [N] fp32 and nearest [N] int32 (a run index); each element has one writer.
 *
 * Any other shape, a metric other than 0 or 1, a null pointer, a workspace that is short or not 16-byte aligned:
 * MMVAE_ERR_ARG, nothing launched.
 */
#ifndef MMVAE_SIL_H
#define MMVAE_SIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MMVAE_OK /* (the same words as mmvae_hip.h; either header may come first) */
typedef void* mmvae_stream_t; /* hipStream_t */
#define MMVAE_OK 0
#define MMVAE_ERR_ARG 1    /* invalid shape / null pointer / short workspace */
#define MMVAE_ERR_LAUNCH 2 /* hipLaunch reported an error */
#endif

/* Version of THIS library: bumped whenever an entry point is added or a signature changes.
 *   1  rows_workspace_bytes, rows */
#define MMVAE_SIL_ABI_VERSION 1
int mmvae_sil_abi_version(void);
const char* mmvae_sil_build_arch(void);

#define MMVAE_SIL_MAX_D 512
#define MMVAE_SIL_EUCLIDEAN 0
#define MMVAE_SIL_COSINE 1

/* Bytes of workspace mmvae_sil_rows_f32 needs at (N, D): the rows padded to a multiple of 64 rows and to 64 / 128 / 256 /
 * 512 columns, their squared norms and the row -> run map.  A multiple of 16; 0 for a refused shape. */
size_t mmvae_sil_rows_workspace_bytes(int N, int D);

/* a, b, s [N] fp32 and nearest [N] int32 of the rows x, as defined above.  Three launches: the padded image with the
 * row -> run map, (metric 0) the norms from the diagonal of the Gram tiles, and the Gram pass. */
int mmvae_sil_rows_f32(int N, int D, const float* x, int64_t ldx, int metric, int R, const int32_t* run_ptr,
                       const int32_t* run_group, float* a, float* b, int32_t* nearest, float* s, void* workspace,
                       size_t workspace_bytes, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_SIL_H */
