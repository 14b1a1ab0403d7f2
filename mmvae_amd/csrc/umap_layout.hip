// Deterministic owner-computes UMAP layout and its uniform start (include/mmvae_umap.h) -> libmmvae_umap.so.
#include "common.h"
#include "../../include/mmvae_umap.h"

namespace {

// ---------------------------------------------------------------- Philox4x32-10
// This library's own copy of the training library's generator (elbo_optim.hip), same word layout: counter words c0, c1 =
// low / high half of the counter, c2, c3 = low / high half of the stream id, key = low / high half of the seed.
struct u32x4 {
    uint32_t x, y, z, w;
};
__device__ __forceinline__ u32x4 philox4x32_10(uint64_t counter, uint64_t stream_id, uint64_t seed) {
    uint32_t c0 = (uint32_t)counter, c1 = (uint32_t)(counter >> 32), c2 = (uint32_t)stream_id,
             c3 = (uint32_t)(stream_id >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}
// Uniform in [2^-25, 1.0] from the top 24 bits of a word, as in elbo_optim.hip.
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__global__ __launch_bounds__(256) void random_init_kernel(int64_t n, float* __restrict__ y, uint64_t seed) {
    const int64_t nq = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        const u32x4 r = philox4x32_10((uint64_t)q, 0, seed);
        const uint32_t rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < n) y[q * 4 + j] = 20.f * u01(rv[j]) - 10.f;
    }
}

__device__ __forceinline__ float clip4(float v) { return fminf(4.f, fmaxf(-4.f, v)); }

// One wave per vertex i; lane l takes edge slots indptr[i] + l, + 64, ...  Every term is formed in fp32 from the OLD
// positions and added into the lane's fp64 sums; the lanes are added by butterfly: a fixed order, and the fp64 sum of
// fp32 terms is exact enough that the order could not be seen in the fp32 result anyway.  Hub vertices of the
// symmetrised graph have rows of thousands of edges: the wave strides over them, nothing is assumed about the length.
template <int C>
__global__ __launch_bounds__(256) void layout_epoch_kernel(int N, const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const int32_t* __restrict__ samples,
                                                           const float* __restrict__ y_old, float* __restrict__ y_new,
                                                           float a, float b, float gamma, int n_epochs, int epoch,
                                                           uint64_t seed) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    float yi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) yi[c] = y_old[(int64_t)i * C + c];
    double sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0.0;
    const int64_t e_end = indptr[i + 1];
    for (int64_t e = indptr[i] + lane; e < e_end; e += 64) {
        const int64_t s = samples[e];
        if ((int64_t)epoch * s / n_epochs <= (int64_t)(epoch - 1) * s / n_epochs) continue;
        const int j = indices[e];
        float diff[C], d2 = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            diff[c] = yi[c] - y_old[(int64_t)j * C + c];
            d2 += diff[c] * diff[c];
        }
        if (d2 > 0.f) {
            const float coeff = (-2.f * a * b * powf(d2, b - 1.f)) / (a * powf(d2, b) + 1.f);
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c] += (double)(2.f * clip4(coeff * diff[c]));
        }
        const u32x4 r0 = philox4x32_10((uint64_t)e * 2, (uint64_t)epoch, seed);
        const u32x4 r1 = philox4x32_10((uint64_t)e * 2 + 1, (uint64_t)epoch, seed);
        const uint32_t word[5] = {r0.x, r0.y, r0.z, r0.w, r1.x};
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int o = (int)(((uint64_t)word[t] * (uint64_t)(unsigned)N) >> 32);
            if (o == i) continue;
            d2 = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                diff[c] = yi[c] - y_old[(int64_t)o * C + c];
                d2 += diff[c] * diff[c];
            }
            if (d2 > 0.f) {
                const float coeff = (2.f * gamma * b) / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += (double)clip4(coeff * diff[c]);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += 4.0;
            }
        }
    }
    const double alpha = 1.0 - (double)(epoch - 1) / (double)n_epochs;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double total = wave_sum_d(sum[c]);
        if (lane == 0) y_new[(int64_t)i * C + c] = (float)((double)yi[c] + alpha * total);
    }
}

}  // namespace

extern "C" int mmvae_umap_random_init_f32(int64_t n, float* y, uint64_t seed, mmvae_stream_t stream) {
    if (n <= 0 || !y) return MMVAE_ERR_ARG;
    const int64_t groups = ((n + 3) / 4 + 255) / 256;
    MMVAE_LAUNCH(random_init_kernel, dim3((unsigned)(groups < 2048 ? groups : 2048)), dim3(256), 0, (hipStream_t)stream, n, y,
                 seed);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_umap_layout_f32(int N, int C, const int64_t* indptr, const int32_t* indices, const int32_t* samples,
                                     float* y0, float* y1, float a, float b, float gamma, int n_epochs, int first, int count,
                                     uint64_t seed, mmvae_stream_t stream) {
    if (N < 1 || (C != 2 && C != 3) || !indptr || !indices || !samples || !y0 || !y1 || y0 == y1) return MMVAE_ERR_ARG;
    if (n_epochs < 1 || first < 1 || count < 0 || (int64_t)first + count - 1 > n_epochs) return MMVAE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 3) / 4)), block(256);
    for (int n = first; n < first + count; ++n) {
        const float* src = ((n - first) & 1) ? y1 : y0;
        float* dst = ((n - first) & 1) ? y0 : y1;
        if (C == 2)
            MMVAE_LAUNCH(layout_epoch_kernel<2>, grid, block, 0, st, N, indptr, indices, samples, src, dst, a, b, gamma,
                         n_epochs, n, seed);
        else
            MMVAE_LAUNCH(layout_epoch_kernel<3>, grid, block, 0, st, N, indptr, indices, samples, src, dst, a, b, gamma,
                         n_epochs, n, seed);
        MMVAE_LAUNCH_CHECK();
    }
    return MMVAE_OK;
}
