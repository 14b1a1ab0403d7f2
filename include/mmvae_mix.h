/*
 * mmvae_mix.h -- C-ABI of libmmvae_mix.so: integration metrics on the latent kNN graph, on the MI355X (gfx950).
 *
 * The pictures of the evaluation (mmvae_umap.h, mmvae_plot.h) show whether the modalities are mixed and the cell types
 * kept apart; this library gives the same answer as a number per cell, from the exact cosine k-nearest-neighbour graph
 * that mmvae_umap_knn_cosine_f32 writes: the local inverse Simpson's index (LISI, Korsunsky et al. 2019) of any category,
 * and the transfer of a label from a cell's neighbours in the other batches.  A library and a version counter of its own
 * (like mmvae_umap.h and mmvae_plot.h), so that it moves neither the training step's ABI nor the UMAP library's.
 *
 * Conventions are those of mmvae_umap.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as void*.  Calls only
 * enqueue work: no allocation, no host synchronisation, no hidden state.  Shapes are validated on the host BEFORE anything
 * is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.  No atomics: bitwise reproducible.
 *
 * The graph.  (idx, dist) [N, k], contiguous, exactly as mmvae_umap_knn_cosine_f32 returns them: idx int32, dist fp32,
 * every row sorted by (distance, index), rank 0 the point itself.  The neighbours of row i are ranks 1 .. k - 1, and
 *
 *     d_j = (double)dist[i][j] - (double)dist[i][1]        j = 1 .. k - 1
 *
 * The shift by the nearest neighbour leaves the normalised weights and the entropy unchanged and keeps the largest weight
 * at exactly 1: the sum of the weights never underflows and every row has a defined result.  All arithmetic is fp64.
 * Limits: 3 <= k <= MMVAE_MIX_MAX_K (the kNN library's limit), N >= 1.  Neighbour indices are trusted to lie in [0, N),
 * as the kNN entry writes them.  Any other shape, a null pointer or a perplexity outside (1, k - 1): MMVAE_ERR_ARG,
 * nothing launched.
 *
 * One wave per row, one rank per lane, four rows to a workgroup; no LDS, no workspace.
 */
#ifndef MMVAE_MIX_H
#define MMVAE_MIX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MMVAE_OK /* (the same words as mmvae_hip.h; either header may come first) */
typedef void* mmvae_stream_t; /* hipStream_t */
#define MMVAE_OK 0
#define MMVAE_ERR_ARG 1    /* invalid shape / null pointer / perplexity out of range */
#define MMVAE_ERR_LAUNCH 2 /* hipLaunch reported an error */
#endif

/* Version of THIS library: bumped whenever an entry point is added or a signature changes.
 *   1  calibrate, lisi, transfer */
#define MMVAE_MIX_ABI_VERSION 1
int mmvae_mix_abi_version(void);
const char* mmvae_mix_build_arch(void);

#define MMVAE_MIX_MAX_K 64
#define MMVAE_MIX_MAX_COLS 8

/* ------------------------------------------------------------------------------------------------------------
 * 1. Calibration  (compute_simpson_index of the LISI paper, with its constants: tol = 1e-5, at most 50 tries)
 *
 *   beta [N] fp64, tries [N] int32.     1 < perplexity < k - 1.
 *
 *   P_j = exp(-beta d_j) / sum_l exp(-beta d_l)          H = log sum_l exp(-beta d_l) + beta sum_l d_l P_l
 *
 * Start at beta = 1, beta_min = -inf, beta_max = +inf.  While |H - log(perplexity)| > tol and fewer than 50 moves have
 * been made: if H is too large, beta_min = beta, then beta <- 2 beta while beta_max is infinite, else (beta + beta_max) / 2;
 * otherwise beta_max = beta, then beta <- beta / 2 while beta_min is -inf, else (beta + beta_min) / 2; H is recomputed
 * after each move.  The row keeps the last beta; tries[i] is the number of moves made.  beta is fp64, so that (2) and (3)
 * reproduce the row's P exactly.  A row whose distances are all equal has uniform P at every beta: it makes its 50 moves
 * and ends at beta = 2^50.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_mix_calibrate_f32(int N, int k, const int32_t* idx, const float* dist, double perplexity, double* beta,
                            int32_t* tries, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * 2. LISI of up to MMVAE_MIX_MAX_COLS code columns in one launch
 *
 *   beta [N] fp64 as written by (1).    codes [n_cols, N] int32, row c at codes + c ldc, ldc >= N.
 *   lisi [n_cols, N] fp32, row c at lisi + c ldl, ldl >= N.     1 <= n_cols <= 8.
 *
 * Any non-negative code is a class -- only equality is used, there is no limit on the number of classes -- and a negative
 * code means unlabelled.  Over the labelled neighbours j of row i, with c_j = codes[c][idx[i][j]]:
 *
 *   m_j = sum_l P_l [c_l = c_j]        S = sum_j P_j m_j / (sum_j P_j)^2        lisi[c][i] = 1 / S
 *
 * The row's own code is not used.  A row with no labelled neighbour gets NaN.  m_j is summed over the ranks l in ascending
 * order: neighbours of one class hold bit-equal masses.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_mix_lisi_f32(int N, int k, const int32_t* idx, const float* dist, const double* beta, int n_cols,
                       const int32_t* codes, int64_t ldc, float* lisi, int64_t ldl, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * 3. Label transfer from the neighbours in the other batches
 *
 *   batch, label [N] int32 (negative = unlabelled).     pred [N] int32, conf, cross [N] fp32.
 *
 * Neighbour j of row i is eligible when batch_j >= 0, batch_j != batch_i and label_j >= 0; a row with batch_i < 0 belongs
 * to no batch, so every labelled neighbour that is in a batch is eligible.  cross_i = the sum of P_j over the eligible
 * neighbours; pred_i = the label with the largest eligible mass (summed over the ranks in ascending order), ties going to
 * the smallest code; conf_i = the winning mass / cross_i (0 / 0 = NaN where every eligible weight has underflowed to 0).
 * With no eligible neighbour: pred_i = -1, conf_i = 0, cross_i = 0.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_mix_transfer_f32(int N, int k, const int32_t* idx, const float* dist, const double* beta, const int32_t* batch,
                           const int32_t* label, int32_t* pred, float* conf, float* cross, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_MIX_H */
