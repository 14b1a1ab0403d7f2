// Segmented histogram + moments of a flat fp32 array (include/mmvae_hist.h) -> libmmvae_hist.so.
#include "common.h"
#include "../../include/mmvae_hist.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int KEYS = 512;       // sign + exponent of an fp32 value, in ascending order of the value
constexpr int MAX_GROUPS = 2048;  // workgroups of the item pass: 8 per CU, each takes a run of consecutive items
constexpr int NSTAT = MMVAE_HIST_STATS;

// fp32 bits -> an unsigned word that ascends with the value (-0.0 directly under +0.0), and back.
__device__ __forceinline__ uint32_t ordered(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ uint32_t unordered(uint32_t u) { return (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u; }

// The number of edges <= v, searched in [lo, hi]: edges[i] <= v for every i < lo and edges[i] > v for every i >= hi hold
// on entry and at every step, so the result is exact whatever range the caller starts from.
__device__ __forceinline__ int count_le(const double* edges, int lo, int hi, double v) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

struct Moments {
    float mn, mx;
    double sum, sq;
    uint32_t fin, nonfin, below, above;
};

// One value per lane, every lane of the wave in the call (`valid`: the lane holds an element).  Bucket counts are
// aggregated in the wave before LDS is touched: the lanes that share the first pending lane's bucket add their count once;
// that repeats while it pays (a round that took fewer than 8 lanes ends it, 4 rounds at most) and what is left goes lane
// by lane.  An all-equal wave costs one LDS add, a spread-out one a single fruitless round.
__device__ __forceinline__ void take(float raw, bool valid, float scale, int n_edges, const double* s_edges,
                                     const uint32_t* s_range, uint32_t* s_hist, Moments& m, int lane) {
    int bucket = -1;
    if (valid) {
        const float v = __fmul_rn(raw, scale);
        const uint32_t bits = __float_as_uint(v);
        if ((bits & 0x7f800000u) == 0x7f800000u) {
            ++m.nonfin;
        } else {
            const double d = (double)v;
            ++m.fin;
            m.mn = fminf(m.mn, v);
            m.mx = fmaxf(m.mx, v);
            m.sum += d;
            m.sq += d * d;  // (exact product: an fp32 square has 48 bits)
            const uint32_t r = s_range[ordered(bits) >> 23];
            const int c = count_le(s_edges, (int)(r & 0xffffu), (int)(r >> 16), d);
            if (c == 0)
                ++m.below;
            else if (c < n_edges)
                bucket = c - 1;
            else if (d == s_edges[n_edges - 1])
                bucket = n_edges - 2;
            else
                ++m.above;
        }
    }
    unsigned long long todo = __ballot(bucket >= 0);
    for (int round = 0; round < 4 && todo; ++round) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(bucket, leader);
        const unsigned long long same = __ballot(bucket == lb) & todo;
        if (lane == leader) atomicAdd(&s_hist[lb], (uint32_t)__popcll(same));
        todo &= ~same;
        if (__popcll(same) < 8) break;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&s_hist[bucket], 1u);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// Workgroup g takes items [g * per, (g + 1) * per).  LDS: the fp64 edges (<= 16 KB), the per-workgroup histogram
// (<= 8 KB), the key table (2 KB) and the waves' partial moments.
__global__ __launch_bounds__(THREADS) void seg_hist_items_kernel(int n_items, int per, const mmvae_hist_item* __restrict__ items,
                                                                 int n_seg, const float* __restrict__ values, float scale,
                                                                 int n_edges, const double* __restrict__ edges,
                                                                 unsigned long long* __restrict__ counts,
                                                                 double* __restrict__ partials,
                                                                 int64_t* __restrict__ seg_first) {
    __shared__ double s_edges[MMVAE_HIST_MAX_EDGES];
    __shared__ uint32_t s_hist[MMVAE_HIST_MAX_EDGES];
    __shared__ uint32_t s_range[KEYS];
    __shared__ double s_red[WAVES][NSTAT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = n_edges - 1;
    for (int i = tid; i < n_edges; i += THREADS) s_edges[i] = edges[i];
    for (int i = tid; i < nb; i += THREADS) s_hist[i] = 0;
    __syncthreads();
    // key k covers the fp32 values whose ordered word starts with k: [count_le(smallest), count_le(largest)] brackets
    // count_le of every one of them (count_le ascends with the value).  Keys of inf / NaN are never looked up.
    for (int k = tid; k < KEYS; k += THREADS) {
        const double vmin = (double)__uint_as_float(unordered((uint32_t)k << 23));
        const double vmax = (double)__uint_as_float(unordered(((uint32_t)k << 23) | 0x7fffffu));
        const bool finite = ((k & 0xff) != (k & 0x100 ? 0xff : 0x00));  // (exponent 255: key 0x1ff above, 0x000 below)
        uint32_t lo = 0, hi = 0;
        if (finite) {
            lo = (uint32_t)count_le(s_edges, 0, n_edges, vmin);
            hi = (uint32_t)count_le(s_edges, 0, n_edges, vmax);
        }
        s_range[k] = lo | (hi << 16);
    }
    __syncthreads();

    const int first = blockIdx.x * per;
    const int last = min(n_items, first + per);
    int cur_seg = -1;        // the segment the LDS histogram belongs to
    uint32_t held = 0;       // elements counted into it since the last flush (its words are 32 bits wide)
    for (int it = first; it < last; ++it) {
        const mmvae_hist_item item = items[it];
        const bool ok = item.len >= 1 && item.len <= MMVAE_HIST_ITEM_ELEMS && item.segment >= 0 && item.segment < n_seg &&
                        item.offset >= 0;
        if (!ok) {  // (uniform over the workgroup) refused: nothing is read; its partials say "no elements"
            if (tid == 0) {
                double* p = partials + (size_t)it * NSTAT;
                p[0] = __builtin_inf();
                p[1] = -__builtin_inf();
                for (int j = 2; j < NSTAT; ++j) p[j] = 0.0;
            }
            continue;
        }
        if (item.segment != cur_seg || held > 0x7fff0000u) {
            if (cur_seg >= 0) {
                __syncthreads();
                for (int b = tid; b < nb; b += THREADS) {
                    const uint32_t c = s_hist[b];
                    if (c) {
                        atomicAdd(&counts[(size_t)cur_seg * nb + b], (unsigned long long)c);
                        s_hist[b] = 0;
                    }
                }
                __syncthreads();
            }
            cur_seg = item.segment;
            held = 0;
        }
        held += (uint32_t)item.len;
        if (tid == 0 && (it == 0 || items[it - 1].segment != item.segment)) seg_first[item.segment] = it;

        const float* base = values + item.offset;
        const int len = item.len;
        // scalar head up to the next 16-byte boundary of the ADDRESS, 16-byte groups, scalar tail
        const int head = min(len, (int)((4u - (uint32_t)(((uintptr_t)base >> 2) & 3u)) & 3u));
        const int n4 = (len - head) >> 2;
        const int tail = len - head - 4 * n4;
        Moments m = {__builtin_inff(), -__builtin_inff(), 0.0, 0.0, 0u, 0u, 0u, 0u};
        const float4* body = reinterpret_cast<const float4*>(base + head);
        for (int j0 = wave * 64; j0 < n4; j0 += THREADS) {  // (the bound is uniform over the wave: every lane makes the calls)
            const int j = j0 + lane;
            const bool valid = j < n4;
            float4 q = {0.f, 0.f, 0.f, 0.f};
            if (valid) q = body[j];
            take(q.x, valid, scale, n_edges, s_edges, s_range, s_hist, m, lane);
            take(q.y, valid, scale, n_edges, s_edges, s_range, s_hist, m, lane);
            take(q.z, valid, scale, n_edges, s_edges, s_range, s_hist, m, lane);
            take(q.w, valid, scale, n_edges, s_edges, s_range, s_hist, m, lane);
        }
        if (wave == 0 && head + tail > 0) {  // at most 6 elements
            const bool valid = lane < head + tail;
            float raw = 0.f;
            if (valid) raw = base[lane < head ? lane : head + 4 * n4 + (lane - head)];
            take(raw, valid, scale, n_edges, s_edges, s_range, s_hist, m, lane);
        }
        // moments of the item: lanes by a fixed tree, waves in order
        float mn = m.mn, mx = m.mx;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_down(mn, o));
            mx = fmaxf(mx, __shfl_down(mx, o));
        }
        const double sum = wave_sum(m.sum), sq = wave_sum(m.sq);
        const uint32_t fin = wave_sum(m.fin), nonfin = wave_sum(m.nonfin), below = wave_sum(m.below),
                       above = wave_sum(m.above);
        if (lane == 0) {
            double* r = s_red[wave];
            r[0] = (double)mn, r[1] = (double)mx, r[2] = (double)fin, r[3] = sum, r[4] = sq, r[5] = (double)nonfin;
            r[6] = (double)below, r[7] = (double)above;
        }
        __syncthreads();
        if (tid == 0) {
            double out[NSTAT];
            for (int j = 0; j < NSTAT; ++j) out[j] = s_red[0][j];
            for (int w = 1; w < WAVES; ++w) {
                out[0] = fmin(out[0], s_red[w][0]);
                out[1] = fmax(out[1], s_red[w][1]);
                for (int j = 2; j < NSTAT; ++j) out[j] += s_red[w][j];
            }
            double* p = partials + (size_t)it * NSTAT;
            for (int j = 0; j < NSTAT; ++j) p[j] = out[j];
        }
        __syncthreads();  // (s_red is rewritten by the next item)
    }
    if (cur_seg >= 0) {
        __syncthreads();
        for (int b = tid; b < nb; b += THREADS) {
            const uint32_t c = s_hist[b];
            if (c) atomicAdd(&counts[(size_t)cur_seg * nb + b], (unsigned long long)c);
        }
    }
}

// One workgroup per segment: thread t sums the partials of the segment's items t, t + 256, ... in that order, the lanes
// are added by a fixed tree and the waves in order.  (Counts up to 2^53 are exact in fp64.)
__global__ __launch_bounds__(THREADS) void seg_hist_reduce_kernel(int n_items, const mmvae_hist_item* __restrict__ items,
                                                                  const double* __restrict__ partials,
                                                                  const int64_t* __restrict__ seg_first,
                                                                  double* __restrict__ stats) {
    __shared__ double s_red[WAVES][NSTAT];
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t first = seg_first[seg];
    double acc[NSTAT] = {__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (first >= 0) {
        for (int64_t it = first + tid; it < n_items && items[it].segment == seg; it += THREADS) {
            const double* p = partials + (size_t)it * NSTAT;
            acc[0] = fmin(acc[0], p[0]);
            acc[1] = fmax(acc[1], p[1]);
#pragma unroll
            for (int j = 2; j < NSTAT; ++j) acc[j] += p[j];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc[0] = fmin(acc[0], __shfl_down(acc[0], o));
        acc[1] = fmax(acc[1], __shfl_down(acc[1], o));
    }
#pragma unroll
    for (int j = 2; j < NSTAT; ++j) acc[j] = wave_sum(acc[j]);
    if (lane == 0)
        for (int j = 0; j < NSTAT; ++j) s_red[wave][j] = acc[j];
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WAVES; ++w) {
            acc[0] = fmin(acc[0], s_red[w][0]);
            acc[1] = fmax(acc[1], s_red[w][1]);
            for (int j = 2; j < NSTAT; ++j) acc[j] += s_red[w][j];
        }
        for (int j = 0; j < NSTAT; ++j) stats[(size_t)seg * NSTAT + j] = acc[j];
    }
}

bool args_ok(int64_t n_items, int n_seg, int n_edges) {
    return n_items >= 1 && n_items <= 0x7fffffff && n_seg >= 1 && n_seg <= n_items && n_edges >= 2 &&
           n_edges <= MMVAE_HIST_MAX_EDGES;
}

}  // namespace

extern "C" int mmvae_hist_abi_version(void) { return MMVAE_HIST_ABI_VERSION; }
extern "C" const char* mmvae_hist_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_hist_workspace_bytes(int64_t n_items, int n_seg, int n_edges) {
    if (!args_ok(n_items, n_seg, n_edges)) return 0;
    const size_t bytes = (size_t)n_items * NSTAT * sizeof(double) + (size_t)n_seg * sizeof(int64_t);
    return (bytes + 15) / 16 * 16;
}

extern "C" int mmvae_hist_segments_f32(int64_t n_items, const mmvae_hist_item* items_dev, int n_seg, const float* values,
                                       float scale, int n_edges, const double* edges_dev, int64_t* counts_out,
                                       double* stats_out, void* workspace, size_t workspace_bytes, mmvae_stream_t stream) {
    if (!args_ok(n_items, n_seg, n_edges)) return MMVAE_ERR_ARG;
    if (!items_dev || !values || !edges_dev || !counts_out || !stats_out || !workspace) return MMVAE_ERR_ARG;
    if (workspace_bytes < mmvae_hist_workspace_bytes(n_items, n_seg, n_edges) || ((uintptr_t)workspace & 15)) return MMVAE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* partials = static_cast<double*>(workspace);
    int64_t* seg_first = reinterpret_cast<int64_t*>(partials + (size_t)n_items * NSTAT);
    (void)hipGetLastError();
    if (hipMemsetAsync(counts_out, 0, (size_t)n_seg * (n_edges - 1) * sizeof(int64_t), st) != hipSuccess) return MMVAE_ERR_LAUNCH;
    if (hipMemsetAsync(seg_first, 0xff, (size_t)n_seg * sizeof(int64_t), st) != hipSuccess) return MMVAE_ERR_LAUNCH;  // -1
    const int per = (int)((n_items + MAX_GROUPS - 1) / MAX_GROUPS);
    const int groups = (int)((n_items + per - 1) / per);
    MMVAE_LAUNCH(seg_hist_items_kernel, dim3((unsigned)groups), dim3(THREADS), 0, st, (int)n_items, per, items_dev, n_seg,
                 values, scale, n_edges, edges_dev, reinterpret_cast<unsigned long long*>(counts_out), partials, seg_first);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(seg_hist_reduce_kernel, dim3((unsigned)n_seg), dim3(THREADS), 0, st, (int)n_items, items_dev, partials,
                 seg_first, stats_out);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
