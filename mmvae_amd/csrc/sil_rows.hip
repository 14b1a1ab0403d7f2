// Silhouette widths of latent embeddings (include/mmvae_sil.h) -> libmmvae_sil.so.
//
// The tile walk is that of knn_gram_kernel (umap_knn.hip): 64 query rows to a workgroup, 16 to a wave as the A operands
// of v_mfma_f32_16x16x4_f32, column tiles of 64 rows through a double-buffered LDS chunk.  The staging code is repeated
// here on purpose (umap_knn.hip is left as it is).  The epilogue differs: the columns arrive in run order, so a query row
// keeps ONE fp64 accumulator, fed per tile from a fixed-order reduction over the 16 lanes that hold its columns, and
// flushed into a (own run) or the running (b, nearest) minimum when the run ends.
#include "common.h"
#include "../../include/mmvae_sil.h"

namespace {

constexpr int SIL_THREADS = 256;
constexpr int WAVES = SIL_THREADS / 64;
constexpr int BM = 16 * WAVES;  // query rows per workgroup: 16 to a wave
constexpr int BN = 64;          // rows of a column tile
constexpr int KC = 64;          // columns of x per staged chunk
constexpr int LDB = KC + 2;     // floats per staged row (bank layout: see umap_knn.hip)

typedef float f32x2 __attribute__((ext_vector_type(2)));

inline int padded_d(int D) { return D <= 64 ? 64 : D <= 128 ? 128 : D <= 256 ? 256 : 512; }
inline int64_t padded_n(int N) { return ((int64_t)N + BM - 1) / BM * BM; }
bool sil_shape_ok(int N, int D) { return N >= 1 && D >= 1 && D <= MMVAE_SIL_MAX_D; }

// ------------------------------------------------------------------------------------------------ 1. padded image
// One wave per row of the padded [Npad, DP] image, lane l the columns l, l + 64, ...: rows past N and columns past D are
// exact zeros.  Cosine: the unit row of knn_unit_rows_kernel.  Lane 0 also writes the row's run (the last run whose start
// is <= the row); a row past N gets the last run, so that it is an ordinary row whose results are never stored.
__global__ __launch_bounds__(256) void sil_rows_kernel(int N, int D, int DP, const float* __restrict__ x, int64_t ldx,
                                                       int metric, int R, const int32_t* __restrict__ run_ptr,
                                                       float* __restrict__ xp, int32_t* __restrict__ row_run,
                                                       int64_t n_pad) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_pad) return;
    float* __restrict__ out = xp + r * DP;
    if (r >= N) {
        for (int c = lane; c < DP; c += 64) out[c] = 0.f;
        if (lane == 0) row_run[r] = R - 1;
        return;
    }
    const float* __restrict__ row = x + r * ldx;
    float scale = 1.f;
    if (metric == MMVAE_SIL_COSINE) {
        double ss = 0.0;
        for (int c = lane; c < D; c += 64) {
            const double v = (double)row[c];
            ss = fma(v, v, ss);
        }
        ss = wave_sum_d(ss);
        scale = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
    }
    if (metric == MMVAE_SIL_COSINE) {
        for (int c = lane; c < DP; c += 64) out[c] = c < D ? row[c] * scale : 0.f;
    } else {
        for (int c = lane; c < DP; c += 64) out[c] = c < D ? row[c] : 0.f;
    }
    if (lane == 0) {
        int lo = 0, hi = R;  // run_ptr[lo] <= r < run_ptr[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (run_ptr[mid] <= (int)r) lo = mid;
            else hi = mid;
        }
        row_run[r] = lo;
    }
}

// ------------------------------------------------------------------------------------------------ 2. squared norms
// n_i = g_ii by the Gram pass's own instruction sequence: one wave per 16 rows, the rows as A and as B operand of the
// same MFMA chain over DP (k ascending from a zero accumulator), the diagonal kept.  Whatever the order of the additions
// inside one MFMA, g_ij of two bit-equal rows then equals n_i and n_j bit for bit.
__global__ __launch_bounds__(256) void sil_norms_kernel(int DP, const float* __restrict__ xp, float* __restrict__ norms,
                                                        int64_t n_pad) {
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int lane = threadIdx.x & 63;
    if (row0 >= n_pad) return;
    const float* __restrict__ p = xp + (row0 + (lane & 15)) * DP + (lane >> 4);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < DP / 4; ++kk) {
        const float v = p[4 * kk];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v, v, acc, 0, 0, 0);
    }
    // accumulator element e: row 4 (lane >> 4) + e, column lane & 15
    const int e = (lane & 15) - 4 * (lane >> 4);
    if (e >= 0 && e < 4) norms[row0 + (lane & 15)] = e == 0 ? acc[0] : e == 1 ? acc[1] : e == 2 ? acc[2] : acc[3];
}

// ------------------------------------------------------------------------------------------------ 3. Gram + run sums
constexpr int STAGE_V = BN * KC / 4 / SIL_THREADS;  // 16-byte groups of a 64 x 64 chunk per thread
struct StagedB {
    f32x4 v[STAGE_V];
};

template <int DP>
__device__ __forceinline__ void stage_load(const float* __restrict__ xp, int tile, int chunk, StagedB& out) {
#pragma unroll
    for (int v = 0; v < STAGE_V; ++v) {
        const int q = threadIdx.x + v * SIL_THREADS;
        out.v[v] = *reinterpret_cast<const f32x4*>(xp + ((int64_t)tile * BN + (q >> 4)) * DP + chunk * KC + 4 * (q & 15));
    }
}
__device__ __forceinline__ void stage_store(float* __restrict__ lds, const StagedB& in) {
#pragma unroll
    for (int v = 0; v < STAGE_V; ++v) {
        const int q = threadIdx.x + v * SIL_THREADS;
        float* __restrict__ dst = lds + (q >> 4) * LDB + 4 * (q & 15);
        *reinterpret_cast<f32x2*>(dst) = f32x2{in.v[v][0], in.v[v][1]};
        *reinterpret_cast<f32x2*>(dst + 2) = f32x2{in.v[v][2], in.v[v][3]};
    }
}

// v + the value of the lane the DPP control names, inside a row of 16 lanes
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// Sum over the 16 lanes of a DPP row, the total in every lane: lane ^ 1, lane ^ 2 (quad permutes), then the mirrored
// half row and the mirrored row, whose sources hold equal values within a quad / half row by then.  Both partners of
// every step add the same two numbers, so the 16 lanes end with the same bits; the order is fixed.
__device__ __forceinline__ float row16_sum(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x140>(v);  // row_mirror
    return v;
}

__device__ __forceinline__ int first_run_not_below(const int32_t* __restrict__ run_group, int R, int g) {
    int lo = 0, hi = R;  // the first run whose group is >= g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (run_group[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Workgroup = 64 query rows, wave w = rows 16 w .. + 15 (lane l: row l & 15, k = 4 kk + (l >> 4)), as in knn_gram_kernel.
// It walks the column tiles from the first column of its first row's group to the last column of its last row's group;
// `run` is the run the walk is in (uniform over the workgroup).  After a tile's last chunk accumulator element e of block
// n is the product of query row 4 (lane >> 4) + e with column 16 n + (lane & 15) of the tile: a lane turns its 16
// products into distances, and for every run that meets the tile sums its columns of that run over n = 0 .. 3, then over
// the 16 lanes of its DPP row (the lanes that hold the other columns of the same four query rows).  The sum joins the
// rows' fp64 accumulators (replicated in those 16 lanes); a run that ends in the tile is flushed.  Rows of another group
// than the run's take no part: the block-diagonal mask.
template <int DP, int METRIC>
__global__ __launch_bounds__(SIL_THREADS) void sil_gram_kernel(const float* __restrict__ xp, const float* __restrict__ norms,
                                                                const int32_t* __restrict__ row_run, int N, int R,
                                                                const int32_t* __restrict__ run_ptr,
                                                                const int32_t* __restrict__ run_group,
                                                                float* __restrict__ a_out, float* __restrict__ b_out,
                                                                int32_t* __restrict__ nearest_out, float* __restrict__ s_out) {
    constexpr int NCH = DP / KC;
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * LDB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * BM + 16 * wave + 4 * (lane >> 4);  // the lane's first query row
    const int cl = lane & 15;

    // the walk
    const int wg_first = blockIdx.x * BM;
    const int wg_last = min(wg_first + BM - 1, N - 1);
    const int g_first = run_group[row_run[wg_first]], g_last = run_group[row_run[wg_last]];
    const int run_begin = __builtin_amdgcn_readfirstlane(first_run_not_below(run_group, R, g_first));
    const int run_end = __builtin_amdgcn_readfirstlane(g_last == 0x7fffffff ? R : first_run_not_below(run_group, R, g_last + 1));
    const int tile_begin = __builtin_amdgcn_readfirstlane(run_ptr[run_begin] / BN);
    const int tile_end = __builtin_amdgcn_readfirstlane((run_ptr[run_end] + BN - 1) / BN);

    float areg[DP / 4];
    {
        const float* __restrict__ arow = xp + (int64_t)(blockIdx.x * BM + 16 * wave + cl) * DP + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < DP / 4; ++kk) areg[kk] = arow[4 * kk];
    }
    int my_run[4], my_group[4], near[4];
    float ni[4];
    double sum[4], av[4], bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        my_run[e] = row_run[row0 + e];
        my_group[e] = run_group[my_run[e]];
        ni[e] = METRIC == MMVAE_SIL_EUCLIDEAN ? norms[row0 + e] : 0.f;
        sum[e] = 0.0;
        av[e] = 0.0;
        bv[e] = __builtin_inf();
        near[e] = -1;
    }

    StagedB p;
    stage_load<DP>(xp, tile_begin, 0, p);
    stage_store(Bs[0], p);
    __syncthreads();

    int run = run_begin;
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        f32x4 acc[4];
        float nj[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            nj[n] = METRIC == MMVAE_SIL_EUCLIDEAN ? norms[tile * BN + 16 * n + cl] : 0.f;
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int buf = ((tile - tile_begin) * NCH + ch) & 1;
            const bool last_chunk = ch == NCH - 1;
            const bool more = !(last_chunk && tile + 1 == tile_end);
            if (more) stage_load<DP>(xp, last_chunk ? tile + 1 : tile, last_chunk ? 0 : ch + 1, p);
            const float* __restrict__ B = Bs[buf] + cl * LDB + (lane >> 4);
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                float bw[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) bw[n] = B[16 * n * LDB + 4 * kk];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[ch * (KC / 4) + kk], bw[n], acc[n], 0, 0, 0);
            }
            if (more) stage_store(Bs[buf ^ 1], p);
            if (last_chunk) {
                const int t0 = tile * BN, t1 = t0 + BN;
                float d[4][4];  // [n][e]
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int col = t0 + 16 * n + cl;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v;
                        if (METRIC == MMVAE_SIL_EUCLIDEAN) v = sqrtf(fmaxf((ni[e] + nj[n]) - 2.f * acc[n][e], 0.f));
                        else v = fmaxf(1.f - acc[n][e], 0.f);
                        d[n][e] = col == row0 + e ? 0.f : v;  // the row itself is no member of its run's sum
                    }
                }
                while (run < run_end) {
                    const int p0 = run_ptr[run], p1 = run_ptr[run + 1];
                    if (p0 >= t1) break;
                    const int g = run_group[run];
                    const int count = p1 - p0;
                    const bool ends = p1 <= t1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = 0.f;
#pragma unroll
                        for (int n = 0; n < 4; ++n) {
                            const int col = t0 + 16 * n + cl;
                            v += (col >= p0 && col < p1) ? d[n][e] : 0.f;
                        }
                        v = row16_sum(v);
                        if (my_group[e] == g) {
                            sum[e] += (double)v;
                            if (ends) {
                                if (my_run[e] == run) {
                                    av[e] = count > 1 ? sum[e] / (double)(count - 1) : 0.0;
                                } else {
                                    const double m = sum[e] / (double)count;
                                    if (m < bv[e]) {
                                        bv[e] = m;
                                        near[e] = run;
                                    }
                                }
                            }
                        }
                        if (ends) sum[e] = 0.0;
                    }
                    if (!ends) break;
                    ++run;
                }
            }
            __syncthreads();
        }
    }
    if (cl == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = row0 + e;
            if (row < N) {
                const bool alone = near[e] < 0;  // the group has no other run
                const double nan = __builtin_nan("");
                const double bb = alone ? nan : bv[e];
                const double top = fmax(av[e], bb);
                const bool single = run_ptr[my_run[e] + 1] - run_ptr[my_run[e]] == 1;
                double sv = nan;
                if (!alone) sv = (single || top == 0.0) ? 0.0 : (bb - av[e]) / top;
                a_out[row] = (float)av[e];
                b_out[row] = (float)bb;
                nearest_out[row] = near[e];
                s_out[row] = (float)sv;
            }
        }
    }
}

template <int DP, int METRIC>
int launch_gram(int N, int R, const float* xp, const float* norms, const int32_t* row_run, const int32_t* run_ptr,
                const int32_t* run_group, float* a, float* b, int32_t* nearest, float* s, hipStream_t st) {
    MMVAE_LAUNCH((sil_gram_kernel<DP, METRIC>), dim3((unsigned)(padded_n(N) / BM)), dim3(SIL_THREADS), 0, st, xp, norms,
                 row_run, N, R, run_ptr, run_group, a, b, nearest, s);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

template <int METRIC>
int launch_metric(int DP, int N, int R, const float* xp, const float* norms, const int32_t* row_run, const int32_t* run_ptr,
                  const int32_t* run_group, float* a, float* b, int32_t* nearest, float* s, hipStream_t st) {
    switch (DP) {
        case 64: return launch_gram<64, METRIC>(N, R, xp, norms, row_run, run_ptr, run_group, a, b, nearest, s, st);
        case 128: return launch_gram<128, METRIC>(N, R, xp, norms, row_run, run_ptr, run_group, a, b, nearest, s, st);
        case 256: return launch_gram<256, METRIC>(N, R, xp, norms, row_run, run_ptr, run_group, a, b, nearest, s, st);
        default: return launch_gram<512, METRIC>(N, R, xp, norms, row_run, run_ptr, run_group, a, b, nearest, s, st);
    }
}

}  // namespace

extern "C" int mmvae_sil_abi_version(void) { return MMVAE_SIL_ABI_VERSION; }
extern "C" const char* mmvae_sil_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_sil_rows_workspace_bytes(int N, int D) {
    if (!sil_shape_ok(N, D)) return 0;
    const size_t n_pad = (size_t)padded_n(N);
    return n_pad * (size_t)padded_d(D) * sizeof(float) + n_pad * sizeof(float) + n_pad * sizeof(int32_t);
}

extern "C" int mmvae_sil_rows_f32(int N, int D, const float* x, int64_t ldx, int metric, int R, const int32_t* run_ptr,
                                  const int32_t* run_group, float* a, float* b, int32_t* nearest, float* s, void* workspace,
                                  size_t workspace_bytes, mmvae_stream_t stream) {
    if (!sil_shape_ok(N, D)) return MMVAE_ERR_ARG;
    if (metric != MMVAE_SIL_EUCLIDEAN && metric != MMVAE_SIL_COSINE) return MMVAE_ERR_ARG;
    if (R < 1 || R > N || ldx < D) return MMVAE_ERR_ARG;
    if (!x || !run_ptr || !run_group || !a || !b || !nearest || !s || !workspace) return MMVAE_ERR_ARG;
    if (workspace_bytes < mmvae_sil_rows_workspace_bytes(N, D) || !aligned16(workspace)) return MMVAE_ERR_ARG;
    const int DP = padded_d(D);
    const int64_t n_pad = padded_n(N);
    float* xp = static_cast<float*>(workspace);
    float* norms = xp + n_pad * DP;
    int32_t* row_run = reinterpret_cast<int32_t*>(norms + n_pad);
    hipStream_t st = (hipStream_t)stream;
    MMVAE_LAUNCH(sil_rows_kernel, dim3((unsigned)(n_pad / 4)), dim3(256), 0, st, N, D, DP, x, ldx, metric, R, run_ptr, xp,
                 row_run, n_pad);
    MMVAE_LAUNCH_CHECK();
    if (metric == MMVAE_SIL_EUCLIDEAN) {
        MMVAE_LAUNCH(sil_norms_kernel, dim3((unsigned)((n_pad / 16 + 3) / 4)), dim3(256), 0, st, DP, xp, norms, n_pad);
        MMVAE_LAUNCH_CHECK();
        return launch_metric<MMVAE_SIL_EUCLIDEAN>(DP, N, R, xp, norms, row_run, run_ptr, run_group, a, b, nearest, s, st);
    }
    return launch_metric<MMVAE_SIL_COSINE>(DP, N, R, xp, norms, row_run, run_ptr, run_group, a, b, nearest, s, st);
}
