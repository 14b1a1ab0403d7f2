// Exact cosine k-nearest-neighbour graph and the per-row fuzzy-set pass (include/mmvae_umap.h) -> libmmvae_umap.so.
#include "common.h"
#include "../../include/mmvae_umap.h"

namespace {

constexpr int KNN_THREADS = 256;  // 4 waves: three such workgroups share a CU, each behind its own barriers, and 64-row
                                  // work items spread more evenly over 256 CUs than 128-row ones did (29.0 against
                                  // 34.6 ms at N = 100 000, D = 128: profiles/umap.txt)
constexpr int WAVES = KNN_THREADS / 64;
constexpr int BM = 16 * WAVES;    // query rows per workgroup: 16 to a wave
constexpr int BN = 64;            // rows of a column tile = candidates a query row meets per tile, one per lane
constexpr int KC = 64;            // columns of x per staged chunk
constexpr int LDB = KC + 2;       // floats per staged row: the 32 lanes of half an MFMA operand read (16 rows r, k = 0 / 1)
                                  // hit the 32 banks (2 r + k) % 32 once each (as in cell_stats.hip)
constexpr int LDT = BN + 4;       // floats per row of a wave's 16 x 64 transposition tile: the four row groups of an
                                  // accumulator store fall on banks 16 apart, two lanes per bank -- the minimum for 64 lanes
constexpr uint64_t KEY_NONE = ~0ull;

typedef float f32x2 __attribute__((ext_vector_type(2)));

inline int padded_d(int D) { return D <= 64 ? 64 : D <= 128 ? 128 : D <= 256 ? 256 : 512; }
inline int64_t padded_n(int N) { return ((int64_t)N + BM - 1) / BM * BM; }

bool knn_shape_ok(int N, int D, int k) {
    return D >= 1 && D <= MMVAE_UMAP_MAX_D && k >= 2 && k <= MMVAE_UMAP_MAX_K && N > k;
}

// ------------------------------------------------------------------------------------------------ 1. unit rows
// One wave per row of the padded [Npad, DP] image; lane l takes columns l, l + 64, ... with scalar loads, so neither the
// leading dimension nor D has to be a multiple of anything.  Rows past N and columns past D are exact zeros.
__global__ __launch_bounds__(256) void knn_unit_rows_kernel(int N, int D, int DP, const float* __restrict__ x, int64_t ldx,
                                                            float* __restrict__ xn, int64_t n_pad) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_pad) return;
    float* __restrict__ out = xn + r * DP;
    if (r >= N) {
        for (int c = lane; c < DP; c += 64) out[c] = 0.f;
        return;
    }
    const float* __restrict__ row = x + r * ldx;
    double ss = 0.0;
    for (int c = lane; c < D; c += 64) {
        const double v = (double)row[c];
        ss = fma(v, v, ss);
    }
    ss = wave_sum_d(ss);
    const float inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
    for (int c = lane; c < DP; c += 64) out[c] = c < D ? row[c] * inv : 0.f;
}

// ------------------------------------------------------------------------------------------------ 2. Gram + top-k
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up1_u64(uint64_t v) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, 1, 64);
    const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), 1, 64);
    return ((uint64_t)hi << 32) | lo;
}

constexpr int STAGE_V = BN * KC / 4 / KNN_THREADS;  // 16-byte groups of a 64 x 64 chunk per thread
struct StagedB {
    f32x4 v[STAGE_V];
};

// Thread t stages the 16-byte groups t, t + KNN_THREADS, ... of the tile's chunk (16 groups to a row): the image is
// padded, every load is whole.
template <int DP>
__device__ __forceinline__ void stage_load(const float* __restrict__ xn, int tile, int chunk, StagedB& out) {
#pragma unroll
    for (int v = 0; v < STAGE_V; ++v) {
        const int q = threadIdx.x + v * KNN_THREADS;
        out.v[v] = *reinterpret_cast<const f32x4*>(xn + ((int64_t)tile * BN + (q >> 4)) * DP + chunk * KC + 4 * (q & 15));
    }
}
__device__ __forceinline__ void stage_store(float* __restrict__ lds, const StagedB& in) {
#pragma unroll
    for (int v = 0; v < STAGE_V; ++v) {
        const int q = threadIdx.x + v * KNN_THREADS;
        float* __restrict__ dst = lds + (q >> 4) * LDB + 4 * (q & 15);
        *reinterpret_cast<f32x2*>(dst) = f32x2{in.v[v][0], in.v[v][1]};
        *reinterpret_cast<f32x2*>(dst + 2) = f32x2{in.v[v][2], in.v[v][3]};
    }
}

// Workgroup = 64 query rows, wave w = rows 16 w .. + 15 of them, held in registers for the whole launch as the A
// operands of v_mfma_f32_16x16x4_f32 (lane l: row l & 15, k = 4 kk + (l >> 4)).  Column tiles of 64 rows stream through a
// double-buffered LDS chunk; the next chunk's global loads are issued ahead of the products and stored behind them: one
// barrier per chunk.  After a tile's last chunk the wave turns its four 16 x 16 accumulators through its own LDS tile so
// that lane l holds candidate column l of one query row at a time, and merges them into the row's sorted list (lane =
// rank): a candidate is looked at only if it beats the row's current k-th key, which after the first few tiles is rare
// (about k ln(N / k) insertions per row in all), so the common case per row and tile is one compare and one ballot.
// Keys: (bits of the distance + 1) << 32 | column, the point itself 0 << 32 | row: unsigned order = (distance, index)
// order with the point first whatever duplicates it has.
template <int DP>
__global__ __launch_bounds__(KNN_THREADS) void knn_gram_kernel(const float* __restrict__ xn, int N, int k,
                                                                int32_t* __restrict__ idx, float* __restrict__ dist) {
    constexpr int NCH = DP / KC;
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * LDB];
    __shared__ __attribute__((aligned(16))) float Ts[WAVES][16 * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * BM + 16 * wave;
    const int ntiles = (N + BN - 1) / BN;

    float areg[DP / 4];
    {
        const float* __restrict__ arow = xn + (int64_t)(row0 + (lane & 15)) * DP + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < DP / 4; ++kk) areg[kk] = arow[4 * kk];
    }
    uint64_t key[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) key[r] = KEY_NONE;

    StagedB p;
    stage_load<DP>(xn, 0, 0, p);
    stage_store(Bs[0], p);
    __syncthreads();

    float* __restrict__ Tw = Ts[wave];
    for (int tile = 0; tile < ntiles; ++tile) {
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int buf = (tile * NCH + ch) & 1;
            const bool last_chunk = ch == NCH - 1;
            const bool more = !(last_chunk && tile + 1 == ntiles);
            if (more) stage_load<DP>(xn, last_chunk ? tile + 1 : tile, last_chunk ? 0 : ch + 1, p);
            const float* __restrict__ B = Bs[buf] + (lane & 15) * LDB + (lane >> 4);
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                float bv[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) bv[n] = B[16 * n * LDB + 4 * kk];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[ch * (KC / 4) + kk], bv[n], acc[n], 0, 0, 0);
            }
            if (more) stage_store(Bs[buf ^ 1], p);
            if (last_chunk) {
                // accumulator element e of tile n: query row 4 (lane >> 4) + e of the wave, column 16 n + (lane & 15)
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int e = 0; e < 4; ++e) Tw[(4 * (lane >> 4) + e) * LDT + 16 * n + (lane & 15)] = acc[n][e];
                __builtin_amdgcn_wave_barrier();  // (one wave's LDS accesses complete in order; this pins the compiler's)
                const int col = tile * BN + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + r;
                    const float d = fmaxf(1.f - Tw[r * LDT + lane], 0.f);
                    uint64_t c = ((uint64_t)(__float_as_uint(d) + 1u) << 32) | (unsigned)col;
                    if (col == row) c = (uint64_t)(unsigned)row;
                    if (col >= N) c = KEY_NONE;
                    uint64_t thr = readlane_u64(key[r], k - 1);
                    uint64_t todo = __ballot(c < thr);
                    while (todo) {
                        const int src = __ffsll((unsigned long long)todo) - 1;
                        todo &= todo - 1;
                        const uint64_t cv = readlane_u64(c, src);
                        if (cv < thr) {
                            const int pos = __popcll(__ballot(key[r] < cv));
                            const uint64_t up = shfl_up1_u64(key[r]);
                            key[r] = lane < pos ? key[r] : (lane == pos ? cv : up);
                            thr = readlane_u64(key[r], k - 1);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + r;
        if (row < N && lane < k) {
            const unsigned hi = (unsigned)(key[r] >> 32);
            idx[(int64_t)row * k + lane] = (int32_t)(unsigned)key[r];
            dist[(int64_t)row * k + lane] = hi == 0u ? 0.f : __uint_as_float(hi - 1u);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. fuzzy set, per row
// One wave per row, lane = rank.  umap-learn's smooth_knn_dist(local_connectivity = 1, bandwidth = 1): rho = the first
// non-zero distance, sigma by bisection in fp64 (lo = 0, hi = inf, mid = 1; doubling while hi is inf), and
// compute_membership_strengths: 0 for the point itself, 1 where d <= rho, exp(-(d - rho) / sigma) otherwise.
__global__ __launch_bounds__(256) void smooth_knn_kernel(int N, int k, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ dist,
                                                         const double* __restrict__ mean_dist, float* __restrict__ rho,
                                                         float* __restrict__ sigma, float* __restrict__ w) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const bool live = lane < k;
    const float df = live ? dist[(int64_t)i * k + lane] : 0.f;
    const int j = live ? idx[(int64_t)i * k + lane] : -1;
    // the row is sorted: the first non-zero distance is the smallest one
    float r = (live && df > 0.f) ? df : __builtin_inff();
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) r = fminf(r, __shfl_xor(r, m, 64));
    if (r == __builtin_inff()) r = 0.f;
    const double d = (double)df - (double)r;
    const bool counted = live && lane >= 1;
    const double target = log2((double)k);
    double lo = 0.0, hi = __builtin_inf(), mid = 1.0;
    for (int it = 0; it < 64; ++it) {
        double term = 0.0;
        if (counted) term = d > 0.0 ? exp(-(d / mid)) : 1.0;
        const double psum = wave_sum_d(term);
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            if (hi == __builtin_inf()) mid *= 2.0;
            else mid = (lo + hi) / 2.0;
        }
    }
    const double row_mean = wave_sum_d(live ? (double)df : 0.0) / (double)k;
    const double floor_v = 1e-3 * (r > 0.f ? row_mean : mean_dist[0]);
    if (mid < floor_v) mid = floor_v;
    const float s = (float)mid;
    if (lane == 0) {
        rho[i] = r;
        sigma[i] = s;
    }
    if (live) {
        float v;
        if (j == i) v = 0.f;
        else if (d <= 0.0 || s == 0.f) v = 1.f;
        else v = (float)exp(-(d / (double)s));
        w[(int64_t)i * k + lane] = v;
    }
}

template <int DP>
int launch_gram(int N, int k, const float* xn, int32_t* idx, float* dist, hipStream_t st) {
    MMVAE_LAUNCH(knn_gram_kernel<DP>, dim3((unsigned)(padded_n(N) / BM)), dim3(KNN_THREADS), 0, st, xn, N, k, idx, dist);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

}  // namespace

extern "C" int mmvae_umap_abi_version(void) { return MMVAE_UMAP_ABI_VERSION; }
extern "C" const char* mmvae_umap_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_umap_knn_cosine_workspace_bytes(int N, int D, int k) {
    if (!knn_shape_ok(N, D, k)) return 0;
    return (size_t)padded_n(N) * (size_t)padded_d(D) * sizeof(float);
}

extern "C" int mmvae_umap_knn_cosine_f32(int N, int D, int k, const float* x, int64_t ldx, int32_t* idx, float* dist,
                                         void* workspace, size_t workspace_bytes, mmvae_stream_t stream) {
    if (!knn_shape_ok(N, D, k)) return MMVAE_ERR_ARG;
    if (!x || ldx < D || !idx || !dist || !workspace) return MMVAE_ERR_ARG;
    if (workspace_bytes < mmvae_umap_knn_cosine_workspace_bytes(N, D, k) || !aligned16(workspace)) return MMVAE_ERR_ARG;
    const int DP = padded_d(D);
    const int64_t n_pad = padded_n(N);
    float* xn = static_cast<float*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    MMVAE_LAUNCH(knn_unit_rows_kernel, dim3((unsigned)(n_pad / 4)), dim3(256), 0, st, N, D, DP, x, ldx, xn, n_pad);
    MMVAE_LAUNCH_CHECK();
    switch (DP) {
        case 64: return launch_gram<64>(N, k, xn, idx, dist, st);
        case 128: return launch_gram<128>(N, k, xn, idx, dist, st);
        case 256: return launch_gram<256>(N, k, xn, idx, dist, st);
        default: return launch_gram<512>(N, k, xn, idx, dist, st);
    }
}

extern "C" int mmvae_umap_smooth_knn_f32(int N, int k, const int32_t* idx, const float* dist, const double* mean_dist,
                                         float* rho, float* sigma, float* w, mmvae_stream_t stream) {
    if (N < 1 || k < 2 || k > MMVAE_UMAP_MAX_K || !idx || !dist || !mean_dist || !rho || !sigma || !w) return MMVAE_ERR_ARG;
    MMVAE_LAUNCH(smooth_knn_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, N, k, idx, dist,
                 mean_dist, rho, sigma, w);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
