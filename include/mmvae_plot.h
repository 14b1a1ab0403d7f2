/*
 * mmvae_plot.h -- C-ABI of libmmvae_plot.so: category scatter plots of an embedding, rasterised on the MI355X (gfx950).
 *
 * The reference's plot_category (runners/umap_predictions.py:165-253) builds a pandas frame of all points, shuffles it,
 * maps an RGBA tuple onto every row and hands it to plt.scatter(s=1, alpha=0.5): seconds to minutes of host time per
 * image.  Here the picture is two passes on the device: every point adds 1 to the pixels of its marker in the count plane
 * of its class (integer atomics), and one lane per pixel turns the class counts into a colour.  A library and a version
 * counter of its own, like mmvae_stats.h, mmvae_disc.h, mmvae_umap.h, mmvae_hist.h and mmvae_prep.h: the training step's
 * ABI does not move.
 *
 * Conventions are those of mmvae_hip.h: extern "C", DEVICE pointers (the one exception, the eight view words, is named
 * `view_host`), `stream` a hipStream_t passed as void*.  Calls only enqueue work: no allocation, no host
 * synchronisation, no hidden state.  Arguments are validated on the host BEFORE anything is launched.  Return value:
 * MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 */
#ifndef MMVAE_PLOT_H
#define MMVAE_PLOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MMVAE_OK /* (the same words as mmvae_hip.h; either header may come first) */
typedef void* mmvae_stream_t; /* hipStream_t */
#define MMVAE_OK 0
#define MMVAE_ERR_ARG 1    /* invalid shape / null pointer / value out of range */
#define MMVAE_ERR_LAUNCH 2 /* hipLaunch reported an error */
#endif

/* Version of THIS library: bumped whenever an entry point is added or a signature changes.
 *   1  count_f32, composite_u8 */
#define MMVAE_PLOT_ABI_VERSION 1
int mmvae_plot_abi_version(void);
const char* mmvae_plot_build_arch(void);

#define MMVAE_PLOT_MAX_CLASSES 16 /* class planes of one picture */
#define MMVAE_PLOT_MAX_MARKER 8   /* the largest marker side, in pixels */
#define MMVAE_PLOT_MAX_SIDE 8192  /* the largest width and height */

/* How mmvae_plot_count_f32 adds: both give the same counts, bit for bit. */
#define MMVAE_PLOT_COUNT_DEFAULT 0   /* the faster of the two as measured (profiles/umap_plot.txt) */
#define MMVAE_PLOT_COUNT_PLAIN 1     /* one no-return integer atomic per point and marker pixel */
#define MMVAE_PLOT_COUNT_AGGREGATE 2 /* lanes of a wave with the same (class, centre pixel) add their number once */

/* ------------------------------------------------------------------------------------------------------------
 * counts_out [n_classes, height, width] uint32: how many markers of each class cover each pixel.
 *
 *   points [n, dims] fp32 with leading dimension ld >= dims (in elements), dims 2 or 3;  codes [n] int32.
 *   view_host: EIGHT fp32 words in HOST memory, read before the call returns: a00 a01 a02 b0 a10 a11 a12 b1.
 *
 * Pixel mapping, every multiply and every add rounded to fp32 on its own (no FMA), in exactly this order:
 *
 *   dims 2:  u = (a00 x + a01 y) + b0                  v = (a10 x + a11 y) + b1            (a02, a12 are not read)
 *   dims 3:  u = ((a00 x + a01 y) + a02 z) + b0        v = ((a10 x + a11 y) + a12 z) + b1
 *
 * The centre pixel is (cx, cy) = (floor(u), floor(v)), x to the right, y DOWN (row cy of the image).  A marker of side
 * m covers columns cx - (m - 1) div 2 .. cx + m div 2 and the rows likewise: for odd m the centre pixel is its middle,
 * for even m the block reaches one pixel further to the right and down than to the left and up.  The point adds 1 to
 * every pixel of that block inside the image.
 *
 * A point is dropped -- it adds nothing anywhere -- when
 *   its code is outside 0 .. n_classes - 1,  or  x, y (or z, dims 3) is NaN or +-inf,  or  u or v is NaN or +-inf,  or
 *   NOT ( -(m div 2) <= floor(u) <= width - 1 + (m - 1) div 2 ),  or the same for floor(v) and height:
 * the last two say that the block misses the image; they are comparisons between fp32 values (the bounds are small
 * integers, exact in fp32), and only a value that passed them is converted to an integer.
 *
 * The entry clears counts_out on the stream, then launches one kernel.  Sums are 32-bit integer atomics only (no
 * floating-point atomics): two calls are bit-identical whatever `mode` says.  Packed inputs (ld == dims, both pointers
 * 16-byte aligned) are read 16 bytes per lane and load; anything else element by element.
 *
 * n < 1 or n > 2^31 - 1, dims not 2 or 3, ld < dims, n_classes outside 1 .. MMVAE_PLOT_MAX_CLASSES, width or height
 * outside 1 .. MMVAE_PLOT_MAX_SIDE, marker outside 1 .. MMVAE_PLOT_MAX_MARKER, mode outside 0 .. 2, a null pointer:
 * MMVAE_ERR_ARG, nothing launched.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_plot_count_f32(int64_t n, int dims, const float* points, int64_t ld, const int32_t* codes, int n_classes,
                         int width, int height, int marker, const float* view_host, int mode, uint32_t* counts_out,
                         mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * rgba_out [height, width, 4] uint8 from counts [n_classes, height, width] and colors [n_classes, 3] fp32 (device):
 * the EXPECTATION of alpha-blending a pixel's markers over the background in a uniformly random order.  With n_c the
 * count of class c and n their sum,
 *
 *   t = (1 - alpha)^n,    channel = (1 - t) * sum_c (n_c / n) colour_c  +  t * background,
 *
 * stored as rint(255 channel) clamped to 0 .. 255, the fourth byte 255 (the picture is opaque).  A pixel with n = 0 is
 * exactly the background: rint(255 background) as the host evaluates it in fp64.  One lane per pixel, evaluated in
 * fp32; class planes are read along the row.
 *
 * n_classes, width or height out of range as above, alpha not in (0, 1], a background channel not in [0, 1], a null
 * pointer, rgba_out not 4-byte aligned: MMVAE_ERR_ARG, nothing launched.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_plot_composite_u8(const uint32_t* counts, int n_classes, int width, int height, const float* colors,
                            float alpha, float bg_r, float bg_g, float bg_b, uint8_t* rgba_out, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_PLOT_H */
