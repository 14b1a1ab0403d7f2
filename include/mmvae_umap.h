/*
 * mmvae_umap.h -- C-ABI of libmmvae_umap.so: the UMAP of latent embeddings on the MI355X (gfx950).
 *
 * The reference ends its evaluation in umap.UMAP(n_neighbors=30, min_dist=0.3, metric="cosine", n_epochs=200)
 * .fit_transform(z) (runners/umap_predictions.py:25-50).  The three device stages of that computation live here, in a
 * library and with a version counter of their own (like mmvae_stats.h and mmvae_disc.h): the exact cosine k-nearest-
 * neighbour graph, the per-row part of the fuzzy simplicial set, and a deterministic stochastic-gradient layout.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers, row-major matrices with a leading dimension in
 * elements, `stream` a hipStream_t passed as void*.  Calls only enqueue work: no allocation, no host synchronisation, no
 * hidden state.  Shapes are validated on the host BEFORE anything is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG /
 * MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_UMAP_H
#define MMVAE_UMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MMVAE_OK /* (the same words as mmvae_hip.h; either header may come first) */
typedef void* mmvae_stream_t; /* hipStream_t */
#define MMVAE_OK 0
#define MMVAE_ERR_ARG 1    /* invalid shape / null pointer / short or misaligned workspace */
#define MMVAE_ERR_LAUNCH 2 /* hipLaunch reported an error */
#endif

/* Version of THIS library: bumped whenever an entry point is added or a signature changes.
 *   1  knn_cosine, smooth_knn, random_init, layout */
#define MMVAE_UMAP_ABI_VERSION 1
int mmvae_umap_abi_version(void);
const char* mmvae_umap_build_arch(void);

#define MMVAE_UMAP_MAX_K 64
#define MMVAE_UMAP_MAX_D 512

/* ------------------------------------------------------------------------------------------------------------
 * 1. Exact cosine k-nearest-neighbour graph  (umap-learn: nearest_neighbors(metric="cosine"), there approximate)
 *
 *   x [N, D] fp32, ldx >= D (rows need not be 16-byte groups)        2 <= k <= 64, k < N, 1 <= D <= 512
 *   idx [N, k] int32, dist [N, k] fp32, both contiguous.  Anything else: MMVAE_ERR_ARG, nothing launched.
 *
 * dist(i, j) = max(0, 1 - <u_i, u_j>), u the fp32 unit rows (a zero-norm row is the zero vector: distance 1 to every
 * other row).  Every output row is sorted ascending by (distance, index); rank 0 is (i, 0.0f) itself -- umap-learn's
 * n_neighbors counts the point.
 *
 * Two launches.  A row pass writes the unit rows (norm from an fp64 sum of squares) into the workspace, zero-padded to
 * a multiple of 64 columns and of 64 rows.  The Gram pass gives 64 query rows to a workgroup of 4 waves; each wave
 * keeps its 16 query rows in registers as v_mfma_f32_16x16x4_f32 operands (exact fp32, one D-long fmaf chain per pair),
 * the column tiles of 64 rows stream through LDS, and each row's running top-k stays in the wave's registers, one rank
 * per lane, as 64-bit (distance, index) keys -- the N x N matrix never exists.  No atomics: bitwise reproducible.
 * |dist - fp64 cosine distance| <= (2 D + 8) 2^-24.
 * ------------------------------------------------------------------------------------------------------------ */
/* 0 for a shape mmvae_umap_knn_cosine_f32 refuses; otherwise a positive multiple of 16: O(N D). */
size_t mmvae_umap_knn_cosine_workspace_bytes(int N, int D, int k);

int mmvae_umap_knn_cosine_f32(int N, int D, int k, const float* x, int64_t ldx, int32_t* idx, float* dist,
                              void* workspace, size_t workspace_bytes, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * 2. Per-row part of the fuzzy simplicial set  (umap-learn: smooth_knn_dist(local_connectivity=1, bandwidth=1) and
 *    compute_membership_strengths)
 *
 *   idx, dist [N, k] as written by (1).   mean_dist: DEVICE double[1], the mean of all N k distances (the floor of a
 *   row without a non-zero distance).     rho, sigma [N] fp32, w [N, k] fp32.
 *
 * rho_i = the smallest non-zero distance of row i (0 when there is none).  sigma_i: up to 64 bisection steps on
 * sum_{j >= 1} exp(-max(d_ij - rho_i, 0) / sigma) = log2(k), stopped at 1e-5, in fp64; floored at 1e-3 x the row mean
 * when rho_i > 0, else 1e-3 x mean_dist.  w_ij = exp(-max(d_ij - rho_i, 0) / sigma_i), 0 where idx_ij == i.
 * One wave per row, one rank per lane.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_umap_smooth_knn_f32(int N, int k, const int32_t* idx, const float* dist, const double* mean_dist, float* rho,
                              float* sigma, float* w, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * 3. Layout
 *
 * Uniform start: y[m] = 20 u01(word m % 4 of philox4x32_10(counter m / 4, stream 0, seed)) - 10, u01 the 24-bit uniform
 * of the training library's generator (the same Philox word layout; tests/philox_mirror.py mirrors it).
 */
int mmvae_umap_random_init_f32(int64_t n, float* y, uint64_t seed, mmvae_stream_t stream);

/* Epochs first .. first + count - 1 (1-based, within 1 .. n_epochs) of the owner-computes layout.
 *
 *   indptr [N + 1] int64, indices [nnz] int32, samples [nnz] int32: the pruned symmetric graph as CSR and, for every
 *   directed edge slot e, its sample count s_e in 1 .. n_epochs.     y0, y1 [N, C] fp32 contiguous, C in {2, 3}.
 *
 * Epoch n reads one buffer and writes the other, starting with y0 -> y1: after `count` epochs the result is in y1 when
 * count is odd and in y0 when it is even.  Edge e is active in epoch n iff (n s_e) div n_epochs > ((n - 1) s_e) div
 * n_epochs.  Vertex i adds, over its active edges i -> j, 2 clip(c (y_i - y_j)), c = -2 a b d2^(b-1) / (a d2^b + 1)
 * (0 at d2 = 0), and for t = 0 .. 4 the repulsion from o = (word * N) >> 32, word = word t % 4 of philox4x32_10(counter
 * 2 e + t / 4, stream n, seed): clip(2 gamma b / ((0.001 + d2)(a d2^b + 1)) (y_i - y_o)), 4 per component at d2 = 0,
 * nothing when o == i; clip is to +-4; then y_i <- y_i + (1 - (n - 1) / n_epochs) * sum.  Terms in fp32, their sum in
 * fp64.  One wave per vertex, the lanes stride over its edges: no atomics, no races, a pure function of the inputs.
 * One launch per epoch.
 */
int mmvae_umap_layout_f32(int N, int C, const int64_t* indptr, const int32_t* indices, const int32_t* samples,
                          float* y0, float* y1, float a, float b, float gamma, int n_epochs, int first, int count,
                          uint64_t seed, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_UMAP_H */
