// Integration metrics on the latent kNN graph (include/mmvae_mix.h) -> libmmvae_mix.so: the perplexity calibration of
// LISI, the inverse Simpson's index of up to eight code columns, and the label transfer from the other batches.
//
// All three kernels have the shape of smooth_knn_kernel (umap_knn.hip): one wave per row, four rows to a workgroup,
// lane = rank, every sum an fp64 butterfly that leaves the same bits in all 64 lanes -- so the calibration loop is
// uniform across the wave.  No LDS, no atomics, no workspace.
#include "common.h"
#include "../../include/mmvae_mix.h"

namespace {

constexpr double MIX_TOL = 1e-5;   // compute_simpson_index of the LISI paper
constexpr int MIX_MAX_TRIES = 50;  //
constexpr int ROWS_PER_BLOCK = 4;

__device__ __forceinline__ double readlane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_xor_d(double v, int m) { return __shfl_xor(v, m, 64); }

// d_j = dist[i][j] - dist[i][1] of the lane's rank (0 on the lanes that hold no neighbour: rank 0 and ranks >= k)
__device__ __forceinline__ double shifted_distance(const float* __restrict__ dist, int64_t i, int k, int lane, bool nb) {
    const float df = lane < k ? dist[i * k + lane] : 0.f;
    const float d1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(df), 1));
    return nb ? (double)df - (double)d1 : 0.0;
}

// P_j of the lane's rank at `beta` (0 on the other lanes); `sum` = sum_l exp(-beta d_l) >= 1, since d_1 = 0
__device__ __forceinline__ double weights(double beta, double d, bool nb, double& sum) {
    const double e = nb ? exp(-beta * d) : 0.0;
    sum = wave_sum_d(e);
    return e / sum;
}

__device__ __forceinline__ double entropy(double beta, double d, bool nb) {
    double sum;
    const double p = weights(beta, d, nb, sum);
    return log(sum) + beta * wave_sum_d(d * p);
}

// ------------------------------------------------------------------------------------------------ 1. calibration
__global__ __launch_bounds__(256) void mix_calibrate_kernel(int N, int k, const float* __restrict__ dist, double log_u,
                                                            double* __restrict__ beta, int32_t* __restrict__ tries) {
    const int64_t i = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= N) return;
    const bool nb = lane >= 1 && lane < k;
    const double d = shifted_distance(dist, i, k, lane, nb);
    double b = 1.0, lo = -__builtin_inf(), hi = __builtin_inf();
    int t = 0;
    double h = entropy(b, d, nb);
    while (fabs(h - log_u) > MIX_TOL && t < MIX_MAX_TRIES) {
        if (h > log_u) {
            lo = b;
            b = hi == __builtin_inf() ? b * 2.0 : (b + hi) / 2.0;
        } else {
            hi = b;
            b = lo == -__builtin_inf() ? b / 2.0 : (b + lo) / 2.0;
        }
        ++t;
        h = entropy(b, d, nb);
    }
    if (lane == 0) {
        beta[i] = b;
        tries[i] = t;
    }
}

// ------------------------------------------------------------------------------------------------ 2. LISI
// The class masses without a histogram: rank l = 1 .. k - 1 in turn broadcasts (c_l, P_l) from its lane -- l is uniform,
// so the broadcast is two scalar reads of a lane -- and every lane whose code matches adds P_l.  Ascending l on every
// lane: the lanes of one class end with bit-equal masses, and the number of classes does not matter.
__global__ __launch_bounds__(256) void mix_lisi_kernel(int N, int k, const int32_t* __restrict__ idx,
                                                       const float* __restrict__ dist, const double* __restrict__ beta,
                                                       int n_cols, const int32_t* __restrict__ codes, int64_t ldc,
                                                       float* __restrict__ lisi, int64_t ldl) {
    const int64_t i = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= N) return;
    const bool nb = lane >= 1 && lane < k;
    const double d = shifted_distance(dist, i, k, lane, nb);
    const int64_t j = nb ? idx[i * k + lane] : 0;
    double sum;
    const double p = weights(beta[i], d, nb, sum);
    for (int c = 0; c < n_cols; ++c) {
        const int code = nb ? codes[c * ldc + j] : -1;
        const bool labelled = code >= 0;
        double m = 0.0;
        for (int l = 1; l < k; ++l) {
            const int cl = __builtin_amdgcn_readlane(code, l);
            if (cl < 0) continue;  // (uniform)
            const double pl = readlane_d(p, l);
            if (code == cl) m += pl;
        }
        const double q = wave_sum_d(labelled ? p * m : 0.0);
        const double t = wave_sum_d(labelled ? p : 0.0);
        const bool any = __ballot(labelled) != 0ull;
        if (lane == 0) lisi[c * ldl + i] = any ? (float)(t * t / q) : __builtin_nanf("");
    }
}

// ------------------------------------------------------------------------------------------------ 3. label transfer
__global__ __launch_bounds__(256) void mix_transfer_kernel(int N, int k, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ dist,
                                                           const double* __restrict__ beta,
                                                           const int32_t* __restrict__ batch,
                                                           const int32_t* __restrict__ label, int32_t* __restrict__ pred,
                                                           float* __restrict__ conf, float* __restrict__ cross) {
    const int64_t i = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= N) return;
    const bool nb = lane >= 1 && lane < k;
    const double d = shifted_distance(dist, i, k, lane, nb);
    const int64_t j = nb ? idx[i * k + lane] : 0;
    double sum;
    const double p = weights(beta[i], d, nb, sum);
    const int bi = batch[i];
    const int bj = nb ? batch[j] : -1;
    const int lj = nb ? label[j] : -1;
    const bool eligible = bj >= 0 && bj != bi && lj >= 0;
    const uint64_t voters = __ballot(eligible);
    const double pe = eligible ? p : 0.0;
    double mass = 0.0;  // of the lane's label
    for (int l = 1; l < k; ++l) {
        if (!((voters >> l) & 1ull)) continue;  // (uniform)
        const int ll = __builtin_amdgcn_readlane(lj, l);
        const double pl = readlane_d(pe, l);
        if (eligible && lj == ll) mass += pl;
    }
    const double total = wave_sum_d(pe);
    // the wave's maximum of (mass, then the smaller code): a total order, so every lane ends with the same pair
    double bm = eligible ? mass : -1.0;
    int bc = eligible ? lj : 0x7fffffff;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double om = shfl_xor_d(bm, m);
        const int oc = __shfl_xor(bc, m, 64);
        if (om > bm || (om == bm && oc < bc)) {
            bm = om;
            bc = oc;
        }
    }
    if (lane == 0) {
        pred[i] = voters ? bc : -1;
        conf[i] = voters ? (float)(bm / total) : 0.f;
        cross[i] = voters ? (float)total : 0.f;
    }
}

bool graph_ok(int N, int k, const void* idx, const void* dist) {
    return N >= 1 && k >= 3 && k <= MMVAE_MIX_MAX_K && idx && dist;
}
inline dim3 row_grid(int N) { return dim3((unsigned)(((int64_t)N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)); }

}  // namespace

extern "C" int mmvae_mix_abi_version(void) { return MMVAE_MIX_ABI_VERSION; }
extern "C" const char* mmvae_mix_build_arch(void) { return "gfx950"; }

extern "C" int mmvae_mix_calibrate_f32(int N, int k, const int32_t* idx, const float* dist, double perplexity,
                                       double* beta, int32_t* tries, mmvae_stream_t stream) {
    if (!graph_ok(N, k, idx, dist) || !beta || !tries) return MMVAE_ERR_ARG;
    if (!(perplexity > 1.0 && perplexity < (double)(k - 1))) return MMVAE_ERR_ARG;  // (a NaN is refused too)
    MMVAE_LAUNCH(mix_calibrate_kernel, row_grid(N), dim3(256), 0, (hipStream_t)stream, N, k, dist, log(perplexity), beta,
                 tries);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_mix_lisi_f32(int N, int k, const int32_t* idx, const float* dist, const double* beta, int n_cols,
                                  const int32_t* codes, int64_t ldc, float* lisi, int64_t ldl, mmvae_stream_t stream) {
    if (!graph_ok(N, k, idx, dist) || !beta || !codes || !lisi) return MMVAE_ERR_ARG;
    if (n_cols < 1 || n_cols > MMVAE_MIX_MAX_COLS || ldc < N || ldl < N) return MMVAE_ERR_ARG;
    MMVAE_LAUNCH(mix_lisi_kernel, row_grid(N), dim3(256), 0, (hipStream_t)stream, N, k, idx, dist, beta, n_cols, codes, ldc,
                 lisi, ldl);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_mix_transfer_f32(int N, int k, const int32_t* idx, const float* dist, const double* beta,
                                      const int32_t* batch, const int32_t* label, int32_t* pred, float* conf, float* cross,
                                      mmvae_stream_t stream) {
    if (!graph_ok(N, k, idx, dist) || !beta || !batch || !label || !pred || !conf || !cross) return MMVAE_ERR_ARG;
    MMVAE_LAUNCH(mix_transfer_kernel, row_grid(N), dim3(256), 0, (hipStream_t)stream, N, k, idx, dist, beta, batch, label,
                 pred, conf, cross);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
