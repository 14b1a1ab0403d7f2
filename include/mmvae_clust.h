/*
 * mmvae_clust.h -- C-ABI of libmmvae_clust.so: k-means clustering of latent embeddings, on the MI355X (gfx950).
 *
 * The kNN-graph metrics (mmvae_mix.h) and the silhouette widths (mmvae_sil.h) ask how well the ANNOTATED classes sit in
 * the embedding.  The last pair of numbers of the scIB report (Luecken et al. 2022), "NMI / ARI cluster / label", asks the
 * converse: does an unsupervised clustering of the embedding recover the annotation?  The clustering is k-means, and its
 * hot path is here: one whole Lloyd iteration per call, and the distance pass of the k-means++ seeding.  A library and a
 * version counter of its own, so that it moves neither the training step's ABI nor any other satellite's.
 *
 * Conventions are those of mmvae_sil.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as void*.  Calls only
 * enqueue work: no allocation, no host synchronisation, no hidden state.  Shapes are validated on the host BEFORE anything
 * is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.  No atomics: every output element has one
 * writer, and two calls on the same inputs give the same bits.
 *
 * Input.  x [N, D] fp32, row i at x + i ldx, ldx >= D, 1 <= D <= MMVAE_CLUST_MAX_D, N >= 1; the columns of a row past D
 * are never read.  centroids [C, D] fp32, dense, 1 <= C <= min(N, MMVAE_CLUST_MAX_C).
 *
 * ---- mmvae_clust_kmeans_step_f32: one Lloyd iteration -----------------------------------------------------------------
 *
 *   score      d2(i, c) = max(0, (n_i + m_c) - 2 g_ic), fp32.  g_ic is the exact-fp32 inner product of row i and centroid
 *              c: one fmaf chain over D in ascending d from zero, as v_mfma_f32_16x16x4_f32 computes it; n_i = g(x_i, x_i)
 *              and m_c = g(c, c) by that same chain.  The Gram form cancels when the rows are far from the origin: the
 *              caller centres them first (as for mmvae_sil.h).
 *   label[i]   the c with the smallest d2(i, c); ties go to the smaller c.  label is READ before it is written, to count
 *              the rows that change: the caller fills it with -1 before the first iteration.
 *   dist2[i]   d2(i, label[i]), fp32.
 *   counts[c]  the number of rows with label c.
 *   new_centroids[c]
 *              the mean of the rows with label c.  The rows are cut into TILES of 64 consecutive rows (the last one
 *              shorter).  Per tile, cluster and column the rows are summed in fp32 in ascending row order; the tile sums
 *              join an fp64 accumulator in ascending tile order.  The tiles are dealt to the workgroups of a grid in
 *              consecutive ranges -- the grid is a function of (N, D, C) alone --; the fp64 sums of the ranges are added in
 *              ascending range order, and the total is divided by the count in fp64 and rounded to fp32 once.  A cluster
 *              without a row keeps centroids[c] bit for bit (and counts[c] = 0).
 *   stats      a 24-byte record, 8-byte aligned:  { double inertia; double shift2; int32 changed; int32 empty; }
 *                inertia   the fp64 sum of dist2: rows ascending inside a range, the ranges' sums in ascending order
 *                shift2    sum_c |new_centroids[c] - centroids[c]|^2 in fp64: per cluster a fixed tree over the columns,
 *                          the clusters in ascending order
 *                changed   the rows whose new label differs from the one read
 *                empty     the clusters without a row
 *
 * x is read from HBM once per call: a tile's scores come from MFMA Gram tiles against the centroids (staged through LDS),
 * and its second read, for the sums, is served by the L2.  Four launches.
 *
 * ---- mmvae_clust_seed_update_f32: the distance pass of k-means++ ------------------------------------------------------
 *
 *   e_i = sum_d (x_id - x_row,d)^2 as ONE fp32 fmaf chain in ascending d from zero -- the direct form, not the Gram form:
 *   the chosen row and every row bit-equal to it get exactly 0 and can never be drawn again.
 *   mind2[i] = e_i when first != 0, else min(mind2[i], e_i).  0 <= row < N.  One launch.
 *
 * Anything else -- a null pointer, C outside [1, min(N, MMVAE_CLUST_MAX_C)], D outside [1, MMVAE_CLUST_MAX_D], ldx < D,
 * row outside [0, N), a workspace that is short or not 16-byte aligned, a stats record that is not 8-byte aligned --:
 * MMVAE_ERR_ARG, nothing launched.
 */
#ifndef MMVAE_CLUST_H
#define MMVAE_CLUST_H

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
 *   1  kmeans_workspace_bytes, kmeans_step, seed_update */
#define MMVAE_CLUST_ABI_VERSION 1
int mmvae_clust_abi_version(void);
const char* mmvae_clust_build_arch(void);

#define MMVAE_CLUST_MAX_D 512
#define MMVAE_CLUST_MAX_C 256
#define MMVAE_CLUST_STATS_BYTES 24

/* Bytes of workspace mmvae_clust_kmeans_step_f32 needs at (N, D, C): the centroids padded to a multiple of 64 rows and
 * to 64 / 128 / 256 / 512 columns with their squared norms, and per workgroup of the grid its fp64 [C, D] sums, its
 * counts, its inertia and its changed rows (the grid shrinks until those sums fit 64 MiB).  A multiple of 16; 0 for a
 * refused shape. */
size_t mmvae_clust_kmeans_workspace_bytes(int N, int D, int C);

/* One Lloyd iteration, as defined above.  label [N] int32 in and out; dist2 [N], new_centroids [C, D] fp32, counts [C]
 * int32 and the stats record out. */
int mmvae_clust_kmeans_step_f32(int N, int D, const float* x, int64_t ldx, int C, const float* centroids,
                                float* new_centroids, int32_t* label, float* dist2, int32_t* counts, void* stats,
                                void* workspace, size_t workspace_bytes, mmvae_stream_t stream);

/* mind2 [N] fp32: the squared distance of every row to row `row`, or the smaller of that and what mind2 held. */
int mmvae_clust_seed_update_f32(int N, int D, const float* x, int64_t ldx, int row, int first, float* mind2,
                                mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_CLUST_H */
