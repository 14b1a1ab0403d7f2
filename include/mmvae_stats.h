/*
 * mmvae_stats.h -- C-ABI of libmmvae_stats.so: evaluation statistics of generated expression on the MI355X (gfx950).
 *
 * libmmvae_hip.so (include/mmvae_hip.h) is the drop-in boundary of the training step and keeps its own version counter;
 * the statistics the reference computes AFTER generation live here, with a counter of their own, so that adding one
 * does not move the training library's ABI.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers, row-major matrices with a leading dimension in
 * elements, `stream` a hipStream_t passed as void*.  Calls only enqueue work: no allocation, no host synchronisation, no
 * hidden state -> hipGraph-capturable.  Shapes are validated on the host BEFORE anything is launched.  Return value:
 * MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_STATS_H
#define MMVAE_STATS_H

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
 *   1  mmvae_stats_row_corr_f32 and its workspace helper */
#define MMVAE_STATS_ABI_VERSION 1
int mmvae_stats_abi_version(void);
const char* mmvae_stats_build_arch(void);

/* ------------------------------------------------------------------------------------------------------------
 * Cell-by-cell correlation of a cis and a cross generation  (replaces calc_correlations, runners/run_correlations.py:
 * 18-60: np.corrcoef of the ROWS of the stacked [n_a + n_b, G] matrix and the nan_to_num means of three of its blocks)
 *
 *   a [n_a, G]   the cis rows          b [n_b, G]   the cross rows (NULL iff n_b == 0)        R = n_a + n_b
 *
 * The two operands are read in place -- they are separate buffers with their own leading dimensions, nothing is
 * stacked.  Accepted: n_a >= 1, n_b >= 0, 2 <= R <= MMVAE_STATS_ROW_CORR_MAX_ROWS, G >= 2, lda / ldb >= G, ldc >= R when
 * `corr` is given, `workspace` 8-byte aligned and at least mmvae_stats_row_corr_workspace_bytes(n_a, n_b, G) long.
 * Anything else: MMVAE_ERR_ARG, nothing launched.
 *
 * corr [R, R] (nullable): np.corrcoef(vstack(a, b)) as fp32, clamped to [-1, 1].  Row i and column i are NaN, diagonal
 *   included, exactly when row i is constant (every value equal to its first; numpy's 0 / 0); the diagonal is exactly
 *   1.0f for every other row; the matrix is bitwise symmetric (one triangle is computed and mirrored).
 * stats: device double[8], required:
 *   [0] cis   mean of nan_to_num(corr[:n_a, :n_a])        [1] cross  mean of nan_to_num(corr[n_a:, n_a:])
 *   [2] comb  mean of nan_to_num(corr[:n_a, n_a:])        [3] 2 comb / (cis + cross)   (IEEE division, unrounded)
 *   [4], [5] the number of constant rows of a and of b    [6], [7] 0
 *   The means are formed from the fp64 values ahead of the fp32 store.  n_b == 0: [1], [2], [3] are NaN.
 *
 * Four launches: a row pass (fp32 row mean m_i from fp64 moments of the values shifted by the row's first element, the
 * constant flag, the fp64 residual sd_i = sum_g (x_ig - m_i) of the centred fp32 values and the row's own cov_ii); a Gram
 * pass over (upper-triangular pairs of 128-row blocks) x (gene splits) on v_mfma_f32_16x16x4_f32 with the centred values
 * staged through LDS, every fp32 chain 64 genes long and flushed into fp64 accumulators; a finishing pass (splits added
 * in split order, cov_ij = S_ij - sd_i sd_j / G, r_ij = cov_ij / sqrt(cov_ii cov_jj)); and one workgroup that adds the
 * block sums.
 * No atomics, fixed summation order: bitwise reproducible, and the same rows give the same `corr` however they are
 * divided between a and b.  |corr - fp64 corrcoef| <= (2 * 64 + 4) * 2^-24 < 8e-6 (DESIGN.md has the derivation).
 * ------------------------------------------------------------------------------------------------------------ */
#define MMVAE_STATS_ROW_CORR_MAX_ROWS 2048
#define MMVAE_STATS_ROW_CORR_STATS 8

/* 0 for a shape mmvae_stats_row_corr_f32 refuses; otherwise a positive multiple of 8. */
size_t mmvae_stats_row_corr_workspace_bytes(int n_a, int n_b, int G);

int mmvae_stats_row_corr_f32(int n_a, int n_b, int G, const float* a, int64_t lda, const float* b, int64_t ldb,
                             float* corr, int64_t ldc, double* stats, void* workspace, size_t workspace_bytes,
                             mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_STATS_H */
