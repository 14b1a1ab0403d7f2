// Connected components and kBET on a neighbour table (include/mmvae_graph.h) -> libmmvae_graph.so.
//
// Connected components.  parent[] is a forest over the vertices with the INVARIANT
//
//     parent[x] <= x at all times, and parent[x] only ever falls: every write is an integer atomicMin.
//
// Sound: a value written into parent[x] is a vertex that an edge path joins to x (a root reached from an endpoint of an
// edge whose other endpoint reaches x), so a tree never leaves its component.  A hook may replace a link x -> p by a lower
// x -> q; the lost tie between x and p is one the edges still state, and the next round reads every edge again.
// Complete: a round that wrote nothing read, for every kept edge, the same root at both ends and, for every vertex, its
// root as its parent -- and since nothing was written during it, what it read is the state it leaves.  A root is a member
// of its tree and no larger than any other member, so it is the component's smallest index: the fixpoint is unique.
// It is reached: the values are bounded below and each writing round lowers one.
//
// No workgroup waits for another.  Every loop has a constant bound (CC_MAX_HOPS, CC_MAX_LINKS, 64); a chase that runs out
// of hops raises `changed` and leaves the rest to the next round.  Every read of parent[] is a relaxed agent-scope atomic
// load: another workgroup's atomicMin lands in memory, not in this CU's L1, and a plain load could go on reading an old
// line.  An old value is an earlier ancestor, never a wrong component -- but the round that proves convergence must see
// what is there.  `changed` is raised by one lane per wave, with a vector atomic.
//
// kBET: the counting has the shape of mix_lisi_kernel (one wave per row, lane = rank, ballot + popcount per batch); the
// p-value is a second, thread-per-row kernel over the stat the first one wrote.
#include <math.h>

#include "common.h"
#include "../../include/mmvae_graph.h"

namespace {

constexpr int CC_MAX_HOPS = 32;   // parent reads of one root chase
constexpr int CC_MAX_LINKS = 8;   // hook attempts of one edge
constexpr int ROWS_PER_BLOCK = 4;
constexpr int GAMMA_MAX_TERMS = 500;
constexpr double GAMMA_EPS = 2.220446049250313e-16;  // 2^-52
constexpr double GAMMA_TINY = 1e-300;

__device__ __forceinline__ int load_parent(const int32_t* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, or the ancestor CC_MAX_HOPS parent reads up (then `gave_up` is set).
__device__ __forceinline__ int chase(const int32_t* parent, int x, bool& gave_up) {
    int p = load_parent(parent, x);
#pragma unroll 1
    for (int h = 1; h < CC_MAX_HOPS && p != x; ++h) {
        x = p;
        p = load_parent(parent, x);
    }
    if (p != x) gave_up = true;
    return p;
}

// one lane of the wave raises the word when any lane asks for it (every lane of the wave reaches this call)
__device__ __forceinline__ void raise_once_per_wave(int32_t* changed, bool flag) {
    if (__ballot(flag) != 0ull && (threadIdx.x & 63) == 0) atomicOr(changed, 1);
}

// ------------------------------------------------------------------------------------------ 1. connected components
// One thread per listed edge (i, idx[i][rank]).
__global__ __launch_bounds__(256) void cc_hook_kernel(int64_t E, int N, int k, const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ codes, int32_t* parent,
                                                      int32_t* changed) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool flag = false;
    if (e < E) {
        const int i = (int)(e / k);
        const int j = idx[e];
        bool kept = j != i && j >= 0 && j < N;  // (an index outside the table is read as no edge, never followed)
        if (kept && codes) {
            const int ci = codes[i];
            kept = ci >= 0 && ci == codes[j];
        }
        if (kept) {
            int a = i, b = j, t = 0;
#pragma unroll 1
            for (; t < CC_MAX_LINKS; ++t) {
                a = chase(parent, a, flag);
                b = chase(parent, b, flag);
                if (a == b) break;
                const int hi = a > b ? a : b, lo = a > b ? b : a;
                const int old = atomicMin(parent + hi, lo);  // lo < hi: parent[hi] <= hi holds
                flag |= old > lo;
                if (old == hi) break;  // hi was a root: the hook stands
                a = old;               // hi had another parent: that one and lo belong together too
                b = lo;
            }
            flag |= t == CC_MAX_LINKS;
        }
    }
    raise_once_per_wave(changed, flag);
}

// One thread per vertex: parent[i] <- the root (or the ancestor CC_MAX_HOPS reads up) it reaches.
__global__ __launch_bounds__(256) void cc_shorten_kernel(int N, int32_t* parent, int32_t* changed) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool flag = false;
    if (t < N) {
        const int i = (int)t;
        const int p = load_parent(parent, i);
        if (p != i) {
            const int r = chase(parent, p, flag);
            if (r < p) flag |= atomicMin(parent + i, r) > r;  // r <= p <= i
        }
    }
    raise_once_per_wave(changed, flag);
}

// ------------------------------------------------------------------------------------------ 2. component sizes
__global__ __launch_bounds__(256) void clear_sizes_kernel(int N, int n_classes, int32_t* __restrict__ size_ws,
                                                          int64_t* __restrict__ class_count,
                                                          int32_t* __restrict__ class_largest,
                                                          int32_t* __restrict__ n_components) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < N) size_ws[t] = 0;
    if (t < n_classes) {
        class_count[t] = 0;
        class_largest[t] = 0;
    }
    if (t == 0) *n_components = 0;
}

// The lanes of `active` that hold the same key as the lowest one of them, and whether this lane is that lowest one.  The
// caller loops while lanes remain: at most 64 turns, one when the wave shares a key.
__device__ __forceinline__ uint64_t same_key_as_first(uint64_t active, int key, int lane, bool& leader) {
    const int first = __builtin_ctzll(active);
    const int first_key = __builtin_amdgcn_readlane(key, first);
    leader = lane == first;
    return __ballot(((active >> lane) & 1ull) && key == first_key);
}

__global__ __launch_bounds__(256) void count_sizes_kernel(int N, const int32_t* __restrict__ root,
                                                          const int32_t* __restrict__ codes, int n_classes,
                                                          int32_t* __restrict__ size_ws, int64_t* __restrict__ class_count,
                                                          int32_t* __restrict__ n_components) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int r = -1, c = -1;
    if (t < N) {
        c = codes ? codes[t] : 0;
        if (c >= n_classes) c = -1;
        r = root[t];
        if (c < 0 || r < 0 || r >= N) r = c = -1;  // unlabelled (or no root of this graph): counted nowhere
    }
    const uint64_t labelled = __ballot(c >= 0);
    uint64_t left = labelled;
#pragma unroll 1
    for (int turn = 0; turn < 64 && left; ++turn) {  // one add per distinct root of the wave
        bool leader;
        const uint64_t same = same_key_as_first(left, r, lane, leader);
        if (leader) atomicAdd(size_ws + r, __builtin_popcountll(same));
        left &= ~same;
    }
    left = labelled;
#pragma unroll 1
    for (int turn = 0; turn < 64 && left; ++turn) {  // one add per distinct class of the wave
        bool leader;
        const uint64_t same = same_key_as_first(left, c, lane, leader);
        if (leader) atomicAdd(reinterpret_cast<unsigned long long*>(class_count + c),
                              (unsigned long long)__builtin_popcountll(same));
        left &= ~same;
    }
    const uint64_t roots = __ballot(c >= 0 && r == (int)t);
    if (roots && lane == 0) atomicAdd(n_components, __builtin_popcountll(roots));
}

__global__ __launch_bounds__(256) void largest_sizes_kernel(int N, const int32_t* __restrict__ root,
                                                            const int32_t* __restrict__ codes, int n_classes,
                                                            const int32_t* __restrict__ size_ws,
                                                            int32_t* __restrict__ class_largest) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    int c = codes ? codes[t] : 0;
    if (c < 0 || c >= n_classes || root[t] != (int)t) return;
    atomicMax(class_largest + c, size_ws[t]);  // (one per component)
}

// ------------------------------------------------------------------------------------------ 3. kBET
// One rounding per operation: no contraction of the product into the subtraction.
__device__ __forceinline__ double chi2_add(double acc, double n_b, double k_i, double f) {
#pragma clang fp contract(off)
    const double e = k_i * f;
    const double d = n_b - e;
    const double sq = d * d;
    const double term = sq / e;
    return acc + term;
}

__global__ __launch_bounds__(256) void kbet_stat_kernel(int N, int k, const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ batch, int n_batches,
                                                        const double* __restrict__ freq, double* __restrict__ stat) {
    const int64_t i = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= N) return;  // (the whole wave)
    const bool nb = lane >= 1 && lane < k;
    const int64_t j = nb ? idx[i * k + lane] : 0;
    const int bj = nb && j >= 0 && j < N ? batch[j] : -1;
    const bool counted = bj >= 0 && bj < n_batches;
    const int k_i = __builtin_popcountll(__ballot(counted));
    double s = 0.0;
#pragma unroll 1
    for (int b = 0; b < n_batches; ++b) {  // (uniform)
        const double f = freq[b];
        if (!(f > 0.0)) continue;
        const int n_b = __builtin_popcountll(__ballot(counted && bj == b));
        s = chi2_add(s, (double)n_b, (double)k_i, f);
    }
    if (lane == 0) stat[i] = k_i > 0 ? s : __builtin_nan("");
}

// Q(a, x) for x > 0, with log_gamma_a = lgamma(a) from the host.
__device__ double gamma_q(double a, double x, double log_gamma_a) {
    const double front = exp(-x + a * log(x) - log_gamma_a);
    if (x < a + 1.0) {  // the series of P
        double ap = a, del = 1.0 / a, sum = del;
#pragma unroll 1
        for (int n = 0; n < GAMMA_MAX_TERMS; ++n) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (fabs(del) < fabs(sum) * GAMMA_EPS) break;
        }
        return 1.0 - sum * front;
    }
    double b = x + 1.0 - a, c = 1.0 / GAMMA_TINY, d = 1.0 / b, h = d;  // modified Lentz
#pragma unroll 1
    for (int n = 1; n <= GAMMA_MAX_TERMS; ++n) {
        const double an = -(double)n * ((double)n - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < GAMMA_TINY) d = GAMMA_TINY;
        c = b + an / c;
        if (fabs(c) < GAMMA_TINY) c = GAMMA_TINY;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < GAMMA_EPS) break;
    }
    return front * h;
}

__global__ __launch_bounds__(256) void kbet_pval_kernel(int N, double a, double log_gamma_a, const double* __restrict__ stat,
                                                        double* __restrict__ pval) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double s = stat[i];
    double p;
    if (s != s) p = s;  // k_i = 0
    else if (s == 0.0) p = 1.0;
    else p = gamma_q(a, 0.5 * s, log_gamma_a);
    pval[i] = p;
}

inline dim3 grid_of(int64_t threads) { return dim3((unsigned)((threads + 255) / 256)); }

}  // namespace

extern "C" int mmvae_graph_abi_version(void) { return MMVAE_GRAPH_ABI_VERSION; }
extern "C" const char* mmvae_graph_build_arch(void) { return "gfx950"; }

extern "C" int mmvae_graph_cc_round_i32(int N, int k, const int32_t* idx, const int32_t* codes, int32_t* parent,
                                        int32_t* changed, mmvae_stream_t stream) {
    if (N < 1 || k < 1 || k > MMVAE_GRAPH_MAX_K || !idx || !parent || !changed) return MMVAE_ERR_ARG;
    const int64_t E = (int64_t)N * k;
    MMVAE_LAUNCH(cc_hook_kernel, grid_of(E), dim3(256), 0, (hipStream_t)stream, E, N, k, idx, codes, parent,
                 changed);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(cc_shorten_kernel, grid_of(N), dim3(256), 0, (hipStream_t)stream, N, parent, changed);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_graph_component_sizes_i32(int N, const int32_t* root, const int32_t* codes, int n_classes,
                                               int32_t* size_ws, int64_t* class_count, int32_t* class_largest,
                                               int32_t* n_components, mmvae_stream_t stream) {
    if (N < 1 || n_classes < 1 || !root || !size_ws || !class_count || !class_largest || !n_components)
        return MMVAE_ERR_ARG;
    if (!codes && n_classes != 1) return MMVAE_ERR_ARG;
    const int64_t widest = N > n_classes ? N : n_classes;
    MMVAE_LAUNCH(clear_sizes_kernel, grid_of(widest), dim3(256), 0, (hipStream_t)stream, N, n_classes, size_ws, class_count,
                 class_largest, n_components);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(count_sizes_kernel, grid_of(N), dim3(256), 0, (hipStream_t)stream, N, root, codes, n_classes, size_ws,
                 class_count, n_components);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(largest_sizes_kernel, grid_of(N), dim3(256), 0, (hipStream_t)stream, N, root, codes, n_classes, size_ws,
                 class_largest);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_graph_kbet_f64(int N, int k, const int32_t* idx, const int32_t* batch, int n_batches,
                                    const double* freq, int dof, double* stat, double* pval, mmvae_stream_t stream) {
    if (N < 1 || k < 2 || k > MMVAE_GRAPH_MAX_K || !idx || !batch || !freq || !stat || !pval) return MMVAE_ERR_ARG;
    if (n_batches < 2 || n_batches > MMVAE_GRAPH_MAX_BATCHES || dof < 1 || dof > n_batches - 1) return MMVAE_ERR_ARG;
    const double a = 0.5 * (double)dof;
    const int64_t row_blocks = ((int64_t)N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    MMVAE_LAUNCH(kbet_stat_kernel, dim3((unsigned)row_blocks), dim3(256), 0, (hipStream_t)stream, N, k, idx, batch, n_batches,
                 freq, stat);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(kbet_pval_kernel, grid_of(N), dim3(256), 0, (hipStream_t)stream, N, a, lgamma(a), stat, pval);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
