/*
 * mmvae_disc.h -- C-ABI of libmmvae_disc.so: the meta-discriminators of the reference (runners/meta_discriminators.py)
 * on the MI355X (gfx950): small sigmoid MLPs trained after the fact to tell from which modality a latent sample or a
 * cross-generated expression matrix came.
 *
 * A third library beside libmmvae_hip.so (include/mmvae_hip.h, the training step) and libmmvae_stats.so
 * (include/mmvae_stats.h, the correlations), with a version counter of its own: adding to it moves neither of theirs.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers, row-major matrices with a leading dimension in
 * elements, `stream` a hipStream_t passed as void*.  Calls only enqueue work: no allocation, no host synchronisation, no
 * hidden state -> hipGraph-capturable.  Shapes are validated on the host BEFORE anything is launched.  Return value:
 * MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_DISC_H
#define MMVAE_DISC_H

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
 *   1  mmvae_disc_tail_f32 and its workspace helper */
#define MMVAE_DISC_ABI_VERSION 1
int mmvae_disc_abi_version(void);
const char* mmvae_disc_build_arch(void);

/* ------------------------------------------------------------------------------------------------------------
 * A discriminator behind its first layer: forward, loss and the whole backward  (create_discriminators / train_md,
 * runners/meta_discriminators.py:16-55, :92-167: Linear(in, H1) . Sigmoid . Linear(H1, H2) . Sigmoid . Linear(H2, 1) .
 * Sigmoid under binary_cross_entropy(reduction="mean")).  The in-wide first layer and its weight gradient are GEMMs of
 * libmmvae_hip.so (mmvae_gemm_f32, NT with bias and TN); this entry takes the first layer's pre-activation.
 *
 *   h1 = sigmoid(pre1)    h2 = sigmoid(h1 W2^T + b2)    s = h2 . W3 + b3    p = sigmoid(s)
 *   loss_row = y min(softplus(-s), 100) + (1 - y) min(softplus(s), 100)        (= torch's -log clamped at -100)
 *   out[0] = mean of loss_row over the B rows       out[1] = fraction of rows with (p > 0.5) == (y > 0.5)
 *
 * Every gradient is that of the MEAN, the 1 / B folded in: ds = (p - y) / B, then the chain back to
 * dpre1 = dh1 h1 (1 - h1); db1 is the column sum of dpre1; dW2 [H2, H1], db2 [H2], dW3 [H2], db3 [1].  Gradients are
 * WRITTEN, never accumulated.
 *
 * Deliberate deviation from fp32 torch: this is torch's fp64 result wherever p (1 - p) >= 1e-12.  Where fp32 sigmoid has
 * already rounded to exactly 0 or 1 (|s| >~ 17), torch's gradient vanishes through the 1e-12 clamp in its backward; here
 * it stays p - y, formed as (1 - y) sigmoid(s) - y sigmoid(-s) so that neither tail cancels, and the derivative of a
 * sigmoid is formed as sigmoid(x) sigmoid(-x).  functional.meta_disc_tail is the tested definition.
 *
 * pre1 [B, H1] with ld1; W2 [H2, H1] contiguous; b2 [H2]; W3 [H2]; b3 [1]; y [B] labels in [0, 1]; p [B] (nullable).
 * Training call:      dpre1 [B, H1] with ldd, db1 [H1], dW2, db2, dW3, db3, y and out all required.
 * Forward-only call:  dpre1 NULL and every gradient pointer NULL; y may be NULL, then out must be NULL and p given.
 *                     p and out carry the same bits as a training call on the same inputs.
 * Accepted: 1 <= B, 1 <= H1 <= 256, 1 <= H2 <= 128, H1 * H2 <= 16384, ld1, ldd >= H1, `workspace` 8-byte aligned and
 * at least mmvae_disc_tail_workspace_bytes(B, H1, H2) long.  Anything else: MMVAE_ERR_ARG, nothing launched.
 *
 * Two launches.  (1) over tiles of MMVAE_DISC_TILE_ROWS rows: a workgroup holds W2 in LDS, takes its rows through the
 * forward and the backward, stores p and dpre1 and writes the tile's partial dW2, db2, dW3, db1, db3, loss sum and hit
 * count into the workspace; past MMVAE_DISC_GRID_CAP tiles a workgroup loops over tiles.  (2) adds the partials in TILE
 * order.  No atomics; inside a tile rows are added in row order: the same inputs give the same bits, whatever the cap.
 * ------------------------------------------------------------------------------------------------------------ */
#define MMVAE_DISC_MAX_H1 256
#define MMVAE_DISC_MAX_H2 128
#define MMVAE_DISC_MAX_W2 16384
#define MMVAE_DISC_TILE_ROWS 16
#define MMVAE_DISC_GRID_CAP 128

/* 0 for a shape mmvae_disc_tail_f32 refuses; otherwise a positive multiple of 8. */
size_t mmvae_disc_tail_workspace_bytes(int B, int H1, int H2);

int mmvae_disc_tail_f32(int B, int H1, int H2, const float* pre1, int64_t ld1, const float* W2, const float* b2,
                        const float* W3, const float* b3, const float* y, float* p, float* out, float* dpre1, int64_t ldd,
                        float* db1, float* dW2, float* db2, float* dW3, float* db3, void* workspace,
                        size_t workspace_bytes, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_DISC_H */
