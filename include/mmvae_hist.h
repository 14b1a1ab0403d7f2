/*
 * mmvae_hist.h -- C-ABI of libmmvae_hist.so: segmented histograms of a flat fp32 array on the MI355X (gfx950).
 *
 * The reference's save_gradients() (models/base_model.py:178-231) hands every parameter's gradient to
 * SummaryWriter.add_histogram: a copy to the host and np.histogram over TensorBoard's 1 549 default edges, per tensor.
 * Here the gradients of one optimiser already lie in one flat arena (mmvae_amd/optim.py), so ONE pass over the arena
 * with a table of segments gives every parameter's histogram and moments.  A library and a version counter of its own,
 * like mmvae_stats.h, mmvae_disc.h and mmvae_umap.h: the training step's ABI does not move.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as void*.  Calls only
 * enqueue work: no allocation, no host synchronisation, no hidden state.  Arguments are validated on the host BEFORE
 * anything is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_HIST_H
#define MMVAE_HIST_H

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
 *   1  workspace_bytes, segments_f32 */
#define MMVAE_HIST_ABI_VERSION 1
int mmvae_hist_abi_version(void);
const char* mmvae_hist_build_arch(void);

#define MMVAE_HIST_ITEM_ELEMS 8192 /* the most elements one work item may cover */
#define MMVAE_HIST_MAX_EDGES 2048  /* the fp64 edge table stays in LDS: 16 KB */
#define MMVAE_HIST_STATS 8         /* doubles per segment in stats_out */

/* A work item: `len` elements of segment `segment`, starting at element `offset` of `values`.  The host cuts every
 * segment into items of 1 .. MMVAE_HIST_ITEM_ELEMS elements; the items of one segment stand together in the table, in
 * order.  Segments may start at any element offset and have any length >= 1.  No element outside [offset, offset + len)
 * of any item is read. */
typedef struct mmvae_hist_item {
    int64_t offset;
    int32_t len;
    int32_t segment;
} mmvae_hist_item;

/* Fields of a stats_out row.  min, max, sum and sum_squares run over the finite values (min = +inf, max = -inf when
 * there is none); num_finite + n_nonfinite = the segment's length; n_below / n_above count the finite values under the
 * first / over the last edge. */
enum {
    MMVAE_HIST_MIN = 0,
    MMVAE_HIST_MAX = 1,
    MMVAE_HIST_NUM_FINITE = 2,
    MMVAE_HIST_SUM = 3,
    MMVAE_HIST_SUM_SQUARES = 4,
    MMVAE_HIST_N_NONFINITE = 5,
    MMVAE_HIST_N_BELOW = 6,
    MMVAE_HIST_N_ABOVE = 7
};

/* 0 for arguments mmvae_hist_segments_f32 refuses; otherwise a positive multiple of 16: 64 n_items + 8 n_seg. */
size_t mmvae_hist_workspace_bytes(int64_t n_items, int n_seg, int n_edges);

/* ------------------------------------------------------------------------------------------------------------
 * counts_out [n_seg, n_edges - 1] int64 and stats_out [n_seg, 8] double of the values v_i = fl32(values[i] * scale)
 * (scale = 1.0f: the value as stored), with the semantics of np.histogram(v.astype(float64), bins=edges):
 *
 *   edges_dev: n_edges STRICTLY ASCENDING doubles, 2 <= n_edges <= MMVAE_HIST_MAX_EDGES (the order is the caller's to
 *   check: the Python wrapper raises ValueError).  Bucket i holds edges[i] <= v < edges[i + 1]; the last bucket also
 *   holds v == edges[n_edges - 1]; a value outside [edges[0], edges[n_edges - 1]], NaN and +-inf go into no bucket.
 *   The comparison is exact (an fp32 value is exact in fp64): the bucket is found by a binary search over the fp64 table
 *   in LDS, started from the range a 512-entry table keyed by the value's sign and exponent gives -- that table is
 *   itself built by binary search over the same edges, so the result is the search's, never an estimate's.
 *
 * Two launches behind two memsets (counts_out and the workspace's segment index are cleared by the entry).  The item
 * pass gives every workgroup a run of consecutive items: bucket counts go wave-aggregated (lanes that share a bucket add
 * their count once) into a per-workgroup LDS histogram, flushed with 64-bit integer atomics when the run's segment
 * changes -- integer sums do not depend on order.  The moments use no floating-point atomics: every item's fp64 partials
 * are written to the workspace (a fixed tree inside the workgroup), and the second launch sums each segment's partials
 * over its items in a fixed order.  Two calls on the same input are bit-identical.
 *
 * n_items < 1, n_seg < 1, n_edges out of range, a null pointer, a workspace shorter than mmvae_hist_workspace_bytes() or
 * not 16-byte aligned: MMVAE_ERR_ARG, nothing launched.  The item table is device memory, which no entry of these
 * libraries reads on the host: an item with len outside 1 .. MMVAE_HIST_ITEM_ELEMS or a segment outside 0 .. n_seg - 1
 * is refused where it is seen -- the item pass skips it, reading nothing.  A segment without a valid item gets zero
 * counts, min = +inf, max = -inf and zeros elsewhere.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_hist_segments_f32(int64_t n_items, const mmvae_hist_item* items_dev, int n_seg, const float* values,
                            float scale, int n_edges, const double* edges_dev, int64_t* counts_out, double* stats_out,
                            void* workspace, size_t workspace_bytes, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_HIST_H */
