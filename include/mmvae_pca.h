/*
 * mmvae_pca.h -- C-ABI of libmmvae_pca.so: the N-scale moments of a principal-component analysis of latent embeddings and
 * of the principal-component regression (PCR) of a covariate on them, on the MI355X (gfx950).
 *
 * scIB's last batch-removal score that is no function of the kNN graph (Luecken et al. 2022, `pc_regression`) asks how
 * much of the embedding's variance a covariate explains: R2 of the covariate on every principal component, weighted by
 * the component's variance.  Everything in it that scales with the number of cells N is here: the centred D x D scatter
 * matrix (with up to eight numeric covariates as extra columns), the per-class column sums of the centred rows, and the
 * projection on the components.  Everything after those moments is D x D work in fp64 on the host (mmvae_amd/pca.py).
 * A library and a version counter of its own, so that it moves neither the training step's ABI nor any other satellite's.
 *
 * Conventions are those of mmvae_clust.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as void*.  Calls only
 * enqueue work: no allocation, no host synchronisation, no hidden state.  Shapes are validated on the host BEFORE anything
 * is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.  No atomics: every output element has one
 * writer, the grid is a function of the shape alone, and two calls on the same inputs give the same bits.
 *
 * Input.  x [N, D] fp32, row i at x + i ldx, ldx >= D, N >= 1; the columns of a row past D are never read.  Optionally
 * y [N, M] fp32 with ldy >= M holds numeric covariates, 0 <= M <= MMVAE_PCA_MAX_COV (M = 0: y is not looked at); the
 * augmented row is a_i = [x_i | y_i] of width W = D + M, 1 <= D, W <= MMVAE_PCA_MAX_D.  mean [W] fp32 is given by the
 * caller.  The centred row is c_iw = fl32(a_iw - mean_w): ONE fp32 subtraction.  Every entry that takes `mean` centres
 * this same way, so that the three outputs are moments of the same numbers.
 *
 * ---- mmvae_pca_group_sums_f64: sorted class sums --------------------------------------------------------------------------
 *
 *   order [run_ptr[C]] int32 lists row indices sorted by class; run_ptr [C + 1] int32 is non-decreasing with
 *   run_ptr[0] = 0 and run_ptr[C] <= N, 1 <= C <= N and C * D <= MMVAE_PCA_MAX_SUMS.  Rows of no class are simply not
 *   listed.  The CONTENTS of both are trusted (as idx is in mmvae_mix.h): every order[k] lies in [0, N).
 *
 *   sums_out[c, d] = sum over k in [run_ptr[c], run_ptr[c + 1]) of c_{order[k], d}, fp64, dense [C, D].  mean = NULL: the
 *   raw x is summed (C = 1 with the identity order gives the column sums the mean is made from).  An empty run gives zeros.
 *
 *   Order of the additions.  The positions k are cut into SEGMENTS at the multiples of MMVAE_PCA_SEGMENT.  Inside a
 *   segment a run's values join an fp64 accumulator, from zero, in ascending k; a run that lies in one segment is that
 *   sum.  A run that crosses segment borders is the sum of its pieces, added from zero in ascending segment order.  There
 *   is no per-workgroup [C, D] table: any C up to N costs the same workspace.  Two launches.
 *
 * ---- mmvae_pca_scatter_f32: the centred scatter matrix ---------------------------------------------------------------------
 *
 *   S_uv = sum_i c_iu c_iv, 0 <= u, v < W, fp64, dense [W, W].
 *
 *   The rows are cut into CHAINS of MMVAE_PCA_CHAIN consecutive rows (the last one shorter).  Within a chain the products
 *   of one (u, v) form ONE fp32 fmaf chain in ascending row order from zero, as v_mfma_f32_16x16x4_f32 computes it.  The
 *   chain results join an fp64 accumulator in ascending chain order.  The chains are dealt to the workgroups in consecutive
 *   ranges -- the grid, (upper-triangular 64 x 64 output tiles) x (row ranges), is a function of (N, W) alone and shrinks
 *   until the workgroups' fp64 tiles fit MMVAE_PCA_PARTIAL_CAP bytes --; the ranges' fp64 partials are added from zero in
 *   ascending range order by a second launch.  Only the tiles on and above the diagonal are computed, of a diagonal tile
 *   only the elements u <= v are kept, and the result is mirrored: S is symmetric bit for bit.
 *
 * ---- mmvae_pca_project_f32: the scores -----------------------------------------------------------------------------------
 *
 *   scores[i, p] = ONE fp32 fmaf chain over d ascending from zero of c_id * components[p, d]; components [P, D] fp32 dense,
 *   1 <= P <= D; scores [N, P] fp32 with row i at scores + i lds, lds >= P (the columns past P are never written).
 *
 * Anything else -- a null pointer, a shape out of range, ld too small, a workspace that is short or not 16-byte aligned --:
 * MMVAE_ERR_ARG, nothing launched.
 */
#ifndef MMVAE_PCA_H
#define MMVAE_PCA_H

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
 *   1  group_sums_workspace_bytes, group_sums, scatter_workspace_bytes, scatter, project */
#define MMVAE_PCA_ABI_VERSION 1
int mmvae_pca_abi_version(void);
const char* mmvae_pca_build_arch(void);

#define MMVAE_PCA_MAX_D 512     /* the widest augmented row, D + M */
#define MMVAE_PCA_MAX_COV 8     /* the most numeric covariates, M */
#define MMVAE_PCA_CHAIN 256     /* rows of one fp32 fmaf chain of the scatter */
#define MMVAE_PCA_SEGMENT 256   /* positions of `order` per segment of the class sums */
#define MMVAE_PCA_PARTIAL_CAP 67108864 /* bytes: the most fp64 partial tiles the scatter's grid may hold (64 MiB) */
#define MMVAE_PCA_MAX_SUMS 1073741824   /* the most elements C * D of sums_out (2^30: 8 GiB of fp64) */

/* Bytes of workspace mmvae_pca_group_sums_f64 needs at (N, D): per segment two fp64 [D] pieces (of the run that enters
 * the segment and of the run that leaves it).  A multiple of 16; 0 for a refused shape. */
size_t mmvae_pca_group_sums_workspace_bytes(int N, int D);

/* The class sums defined above.  mean [D] fp32 or NULL. */
int mmvae_pca_group_sums_f64(int N, int D, const float* x, int64_t ldx, const float* mean, int C, const int32_t* order,
                             const int32_t* run_ptr, double* sums_out, void* workspace, size_t workspace_bytes,
                             mmvae_stream_t stream);

/* Bytes of workspace mmvae_pca_scatter_f32 needs at (N, D, M): one fp64 64 x 64 tile per workgroup of its grid.  A
 * multiple of 16, at most MMVAE_PCA_PARTIAL_CAP; 0 for a refused shape. */
size_t mmvae_pca_scatter_workspace_bytes(int N, int D, int M);

/* The scatter matrix defined above.  y may be NULL when M = 0. */
int mmvae_pca_scatter_f32(int N, int D, const float* x, int64_t ldx, int M, const float* y, int64_t ldy, const float* mean,
                          double* scatter_out, void* workspace, size_t workspace_bytes, mmvae_stream_t stream);

/* The scores defined above. */
int mmvae_pca_project_f32(int N, int D, const float* x, int64_t ldx, const float* mean, int P, const float* components,
                          float* scores, int64_t lds, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_PCA_H */
