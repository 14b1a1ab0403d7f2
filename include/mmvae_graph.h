/*
 * mmvae_graph.h -- C-ABI of libmmvae_graph.so: connected components and kBET on a neighbour table, on the MI355X (gfx950).
 *
 * Two scIB integration numbers that are functions of the latent kNN graph (the one mmvae_umap_knn_cosine_f32 writes and
 * mmvae_mix.h reads): graph connectivity -- per label, the share of its cells in the largest connected component of the
 * graph restricted to that label -- and kBET, a chi-square test of every neighbourhood's batch composition.  Connected
 * components is an entry of its own and takes any [N, k] neighbour table.  A library and a version counter of its own
 * (like mmvae_mix.h), so that it moves neither the training step's ABI nor another satellite's.
 *
 * Conventions are those of mmvae_mix.h: extern "C", DEVICE pointers, `stream` a hipStream_t passed as void*.  Calls only
 * enqueue work: no allocation, no host synchronisation, no hidden state.  Shapes are validated on the host BEFORE anything
 * is launched.  Return value: MMVAE_OK / MMVAE_ERR_ARG / MMVAE_ERR_LAUNCH.
 *
 * The graph.  idx [N, k] int32, contiguous: row i lists neighbours of i in any order.  Self entries and duplicates are
 * allowed and ignored.  Indices are trusted to lie in [0, N), as the kNN entry writes them.  N >= 1, 1 <= k <=
 * MMVAE_GRAPH_MAX_K.  Codes (labels, batches) are int32, negative = unlabelled; a code at or above the entry's class
 * count is read as unlabelled too.
 *
 * Atomics.  (1) and (2) use INTEGER atomics only (min, add, max, or): exact and independent of the order they land in, so
 * their results are bitwise reproducible although the scheduling is not.  (3) uses none.  No workgroup ever waits for
 * another one: no spinning, no tickets, no grid-wide barrier, and every loop inside a kernel has a constant bound.
 */
#ifndef MMVAE_GRAPH_H
#define MMVAE_GRAPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MMVAE_OK /* (the same words as mmvae_hip.h; either header may come first) */
typedef void* mmvae_stream_t; /* hipStream_t */
#define MMVAE_OK 0
#define MMVAE_ERR_ARG 1    /* invalid shape / null pointer / count out of range */
#define MMVAE_ERR_LAUNCH 2 /* hipLaunch reported an error */
#endif

/* Version of THIS library: bumped whenever an entry point is added or a signature changes.
 *   1  cc_round, component_sizes, kbet */
#define MMVAE_GRAPH_ABI_VERSION 1
int mmvae_graph_abi_version(void);
const char* mmvae_graph_build_arch(void);

#define MMVAE_GRAPH_MAX_K 64
#define MMVAE_GRAPH_MAX_BATCHES 64

/* ------------------------------------------------------------------------------------------------------------
 * 1. One round of connected components
 *
 *   codes [N] int32 or NULL.    parent [N] int32, in/out.    changed: one int32 device word.
 *
 * The graph is the undirected union of the listed edges: (i, j) is an edge when i lists j or j lists i.  With codes, an
 * edge is kept only when codes[i] == codes[j] >= 0; an unlabelled vertex is then a singleton.
 *
 * The caller starts from parent[i] = i and clears *changed before a round (or a group of rounds).  A round hooks -- for
 * every kept edge it finds the two current roots and atomicMin's the smaller into the larger one's parent -- and then
 * shortens every vertex's path to the root it reaches.  It sets *changed nonzero when it wrote a lower value anywhere,
 * or gave up a root chase after its fixed number of hops.  The state after a round that left *changed zero is the result:
 * parent[i] is the smallest index of i's component.  That fixpoint is unique: the result is bit-equal on repetition,
 * whatever the number of rounds was.
 *
 * Invariant: parent[x] <= x at all times, and a value only ever falls (every write is an integer atomicMin).
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_graph_cc_round_i32(int N, int k, const int32_t* idx, const int32_t* codes, int32_t* parent, int32_t* changed,
                             mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * 2. Component sizes per class
 *
 *   root [N] int32 as (1) leaves it.    codes [N] int32 or NULL (a single class 0).    1 <= n_classes.
 *   size_ws [N] int32 workspace.    class_count [n_classes] int64.    class_largest [n_classes] int32.
 *   n_components: one int32.
 *
 * The entry clears size_ws and the three outputs itself.  size_ws[r] = the labelled vertices whose root is r;
 * class_count[c] = the vertices of class c; class_largest[c] = the largest size_ws[r] over the roots r of class c (0 for
 * an empty class); *n_components = the labelled roots.  Unlabelled vertices are counted nowhere.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_graph_component_sizes_i32(int N, const int32_t* root, const int32_t* codes, int n_classes, int32_t* size_ws,
                                    int64_t* class_count, int32_t* class_largest, int32_t* n_components,
                                    mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * 3. kBET: chi-square test of the batch composition of every neighbourhood
 *
 *   batch [N] int32 (negative = unlabelled).    2 <= n_batches <= MMVAE_GRAPH_MAX_BATCHES.    freq [n_batches] fp64.
 *   1 <= dof <= n_batches - 1 (the caller passes the number of freq[b] > 0, minus 1).    stat, pval [N] fp64.
 *
 * Rank 0 is the cell itself; the neighbourhood of row i is ranks 1 .. k - 1, so k >= 2.  Per row, in fp64:
 *
 *   n_b = the neighbours with batch code b         k_i = sum_b n_b  (unlabelled neighbours do not count)
 *   e_b = (double)k_i * freq[b]
 *   stat_i = sum over ascending b with freq[b] > 0 of (n_b - e_b)^2 / e_b
 *   pval_i = Q(dof / 2, stat_i / 2)                the regularised upper incomplete gamma function
 *
 * The subtraction, the product, the IEEE division and the sum of every term are each rounded once.  Q is the series of
 * P for x < a + 1 and the modified Lentz continued fraction otherwise, both stopped at relative 2^-52 or after 500
 * terms.  stat_i = 0 gives pval_i = 1; k_i = 0 gives stat_i = pval_i = NaN.
 * ------------------------------------------------------------------------------------------------------------ */
int mmvae_graph_kbet_f64(int N, int k, const int32_t* idx, const int32_t* batch, int n_batches, const double* freq, int dof,
                         double* stat, double* pval, mmvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_GRAPH_H */
