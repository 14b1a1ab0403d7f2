/*
 * mmvae_ckpt.h -- C-ABI of libmmvae_ckpt.so: the device snapshot behind a checkpoint, on the MI355X (gfx950).
 *
 * A checkpoint of a training run wants every parameter, Adam moment, buffer and RNG word as they are at ONE point of the
 * stream, without stopping the captured step.  One launch reads a table of ranges ("jobs") in stream order, writes them
 * back to back into a private device buffer, and computes per range, in the same pass, a position-sensitive 64-bit
 * checksum and a count of non-finite fp32 values.  Training goes on; a worker thread drains the private copy
 * (mmvae_amd/checkpoint.py).  A library and a version counter of its own, like mmvae_stats.h, mmvae_disc.h, mmvae_umap.h,
 * mmvae_hist.h, mmvae_prep.h and mmvae_plot.h: the training step's ABI does not move.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers unless said otherwise, `stream` a hipStream_t passed
 * as void*.  Calls only enqueue work: no allocation, no host synchronisation, no hidden state.  Arguments are validated
 * on the host BEFORE anything is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_CKPT_H
#define MMVAE_CKPT_H

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
 *   1  check_jobs, snapshot */
#define MMVAE_CKPT_ABI_VERSION 1
int mmvae_ckpt_abi_version(void);
const char* mmvae_ckpt_build_arch(void);

#define MMVAE_CKPT_F32 1u            /* job flag: the words are fp32 values, count the non-finite ones */
#define MMVAE_CKPT_CHUNK_WORDS 8192  /* one work item: this many words of one job (a 256-thread workgroup, 8 x 16 B a lane) */
#define MMVAE_CKPT_MAX_GROUPS 2048   /* the grid's cap; the remaining (job, chunk) items are grid-strided */

typedef struct {
  const void* src;   /* 4-byte aligned */
  uint64_t dst_word; /* where the range starts in `dst`, in 32-bit words */
  uint64_t n_words;  /* < 2^32 */
  uint32_t flags;    /* MMVAE_CKPT_F32 or 0 */
  uint32_t reserved; /* 0 */
} mmvae_ckpt_job;    /* 32 B */

/* ------------------------------------------------------------------------------------------------------------
 * The per-job checks, on a table in HOST memory (the table the caller is about to upload; `src` is looked at, never
 * followed).  A misaligned `src`, a NULL `src` with n_words > 0, n_words >= 2^32, a flag bit other than MMVAE_CKPT_F32,
 * a reserved word that is not 0, n_jobs < 0, a NULL table with n_jobs > 0: MMVAE_ERR_ARG.  Otherwise MMVAE_OK, with the
 * largest n_words of the table in *max_words_out (when not NULL; 0 for an empty table): the `max_words` of the launch.
 * mmvae_ckpt_snapshot cannot make these checks itself: its table lies in device memory, where the host does not read.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_ckpt_check_jobs(int n_jobs, const mmvae_ckpt_job* jobs_host, uint64_t* max_words_out);

/* ------------------------------------------------------------------------------------------------------------
 * One launch over all jobs of the DEVICE table `jobs_dev`.  Everything is 32-bit words w_i; for job j, i < n_words:
 *
 *   dst[dst_word + i] = w_i                                               bit for bit (skipped when dst is NULL: the
 *                                                                         digest-only mode that verifies a loaded state)
 *   digest[j][0] = sum_i (w_i + 1) * ((2 i + 1) * 0x9E3779B97F4A7C15)     all arithmetic mod 2^64 (w_i + 1 <= 2^32 is not
 *                                                                         reduced mod 2^32)
 *   digest[j][1] = #{ i : (w_i & 0x7F800000) == 0x7F800000 }              with MMVAE_CKPT_F32, else 0
 *
 * The checksum is a sum in Z / 2^64 added up with integer atomics: every reduction order gives the same bits, two calls
 * on unchanged data give identical digests, and mmvae_amd.checkpoint.snapshot_digest_reference is its numpy mirror.
 * The odd factor 2 i + 1 makes it position-sensitive (two unequal words swapped change it), the + 1 makes a range of
 * zeros depend on its length.  `digest` ([n_jobs][2], 8-byte aligned) is cleared by the call itself, in stream order.
 *
 * `max_words` bounds every job's n_words (mmvae_ckpt_check_jobs hands it out); the device clamps n_words to it, so a
 * table that disagrees copies less, never more.  No word outside [src, src + n_words) is read and none outside
 * dst[dst_word, dst_word + n_words) written, for every 4-byte-aligned src and every dst_word: 16-byte loads and stores
 * run where src and dst + dst_word are congruent mod 16 bytes (a head of up to 3 words and a tail are peeled per chunk),
 * single words otherwise -- with dst itself 16-byte aligned, dst_word = (src / 4) (mod 4) keeps a job on the wide path.  A job
 * whose src is not 4-byte aligned is skipped on the device (its digest stays 0).  Ranges of different jobs must not
 * overlap in dst.
 *
 * n_jobs < 0, jobs_dev NULL with n_jobs > 0, digest NULL or not 8-byte aligned with n_jobs > 0, dst not 4-byte aligned,
 * max_words >= 2^32: MMVAE_ERR_ARG, nothing launched.  n_jobs == 0 and jobs with n_words == 0 are valid.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_ckpt_snapshot(int n_jobs, const mmvae_ckpt_job* jobs_dev, uint64_t max_words, void* dst, uint64_t* digest,
                        mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_CKPT_H */
