/*
 * mmvae_prep.h -- C-ABI of libmmvae_prep.so: raw count chunks (CSR, fp32) -> what the model trains on, on the MI355X
 * (gfx950).
 *
 * The reference's normalize_data() (scripts/data-preprocessing/data_processing_functions.py:12-31) walks a chunk row by
 * row in Python -- one getrow() per cell -- and writes log1p(1e4 * v / rowsum) back into it.  Here ONE launch normalises
 * a whole chunk where it lies in device memory (a wave per row), and hands out the per-cell totals whose mean and
 * standard deviation the reference records as its sanity check (get_data_stats).  A library and a version counter of its
 * own, like mmvae_stats.h, mmvae_disc.h, mmvae_umap.h and mmvae_hist.h: the training step's ABI does not move.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as void*.  Calls only
 * enqueue work: no allocation, no host synchronisation, no hidden state.  Arguments are validated on the host BEFORE
 * anything is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_PREP_H
#define MMVAE_PREP_H

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
 *   1  csr_log1p_norm_i32, csr_log1p_norm_i64 */
#define MMVAE_PREP_ABI_VERSION 1
int mmvae_prep_abi_version(void);
const char* mmvae_prep_build_arch(void);

#define MMVAE_PREP_ROWS_PER_GROUP 4 /* a wave per row, four rows per workgroup */
#define MMVAE_PREP_REG_ELEMS 1024   /* a row of up to this many stored elements stays in registers between its sum and
                                       its transform; a longer one re-reads what lies beyond (an L2 hit) */

/* ------------------------------------------------------------------------------------------------------------
 * In place, per row r with the stored values v[crow[r] .. crow[r + 1]):
 *
 *   s = fl32(sum v)      accumulated in fp64 over a fixed tree (lane l of the row's wave adds elements l, l + 64, ... in
 *                        that order, the 64 partials are added by a fixed butterfly): two calls are bit-identical.  For
 *                        integer counts with a total below 2^24 this is numpy's fp32 row_data.sum() exactly, whatever
 *                        its order; for larger totals it is the correctly rounded sum.
 *   v <- log1p( fl32( fl32(v * target_sum) / s ) )
 *                        the multiply first, then a true IEEE division: the reference's expression order.  No
 *                        reciprocal, no fast-math.  log1p in fp32 within 2 ulp, like log1pf: logf(u) + c / u with
 *                        u = fl(1 + x) and c the exact rounding error of that sum (the library's log1pf costs four times
 *                        the instructions and made the kernel instruction-bound).  With the three roundings before it,
 *                        every element lies within 6 * 2^-24 = 3.6e-7 relative of an fp64 evaluation of the formula.
 *   row_sums_out[r] = s  when row_sums_out is not NULL.
 *
 * A row without stored elements writes nothing but its sum, 0.  DEVIATION from the reference: a row WITH stored elements
 * whose sum is 0 (stored zeros) gets 0.0 in every element; the reference divides by zero there and writes NaN (numpy warns
 * "invalid value encountered in divide"), which is never what a training batch should carry.
 *
 * Column indices are not an argument and are never touched.  crow is read at [0, n_rows] only; no value outside
 * [crow[0], crow[n_rows]) is read or written, and a row pointer outside [0, nnz] is clamped into it before it is used (a
 * malformed table shortens rows, it does not reach outside `values`).  _i32 / _i64: the type of the row pointers.
 *
 * n_rows < 1, n_rows > 2^33 - 4, nnz < 0, crow NULL, values NULL with nnz > 0, target_sum not finite or <= 0:
 * MMVAE_ERR_ARG, nothing launched.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_prep_csr_log1p_norm_i32(int64_t n_rows, int64_t nnz, const int32_t* crow, float* values, float target_sum,
                                  float* row_sums_out, mmvae_stream_t stream);
int mmvae_prep_csr_log1p_norm_i64(int64_t n_rows, int64_t nnz, const int64_t* crow, float* values, float target_sum,
                                  float* row_sums_out, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_PREP_H */
