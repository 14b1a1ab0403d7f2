// log1p-per-10k normalisation of a raw CSR count chunk, in place (include/mmvae_prep.h) -> libmmvae_prep.so.
#include <math.h>

#include "common.h"
#include "../../include/mmvae_prep.h"

namespace {

constexpr int ROWS = MMVAE_PREP_ROWS_PER_GROUP;  // a wave per row
constexpr int THREADS = 64 * ROWS;
constexpr int CACHE = MMVAE_PREP_REG_ELEMS / 64;  // values a lane keeps between the sum and the transform

// log(1 + x) from the hardware logarithm: u = fl(1 + x), c = x - (u - 1) is the rounding error of that sum exactly
// (u - 1 is exact below 2^24, and the error of an addition is a floating-point number), and
// log(1 + x) = log(u) + log(1 + c / u) = log(u) + c / u up to (c / u)^2 / 2 <= 2^-49.  Error: logf's own (<= 1 ulp,
// i.e. <= 2 * 2^-24 relative) plus the last addition's rounding (2^-24): within the 2 ulp asked of log1pf, for 14 + 15
// instructions where the library's log1pf takes 121 -- which made this kernel instruction-bound (profiles/prep.txt).
// u = 0 (-inf), u < 0 and NaN (NaN) and u = inf (inf) take logf's answer as it is.
__device__ __forceinline__ float log1p_f32(float x) {
    const float u = __fadd_rn(1.f, x);
    const float c = __fsub_rn(x, __fsub_rn(u, 1.f));
    const float l = logf(u);
    return (u > 0.f && u < __builtin_inff()) ? __fadd_rn(l, __fdiv_rn(c, u)) : l;
}

// v <- log1p(fl32(fl32(v * t) / s)); 0.0 for a row of stored zeros (`dead`), where the reference writes NaN
__device__ __forceinline__ float transform(float v, float t, float s, bool dead) {
    return dead ? 0.f : log1p_f32(__fdiv_rn(__fmul_rn(v, t), s));
}

// Row starts fall on any element offset, so every access is one dword per lane: a wave instruction covers 256
// consecutive bytes whatever the row's alignment, with no head or tail to peel.
template <typename idx_t>
__global__ __launch_bounds__(THREADS) void csr_log1p_norm_kernel(int64_t n_rows, int64_t nnz, const idx_t* __restrict__ crow,
                                                                 float* __restrict__ values, float target_sum,
                                                                 float* __restrict__ row_sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * ROWS + wave;
    if (row >= n_rows) return;  // (uniform over the wave; there is no workgroup barrier below)
    int64_t start = (int64_t)crow[row], end = (int64_t)crow[row + 1];
    start = start < 0 ? 0 : (start > nnz ? nnz : start);
    end = end < 0 ? 0 : (end > nnz ? nnz : end);
    const int64_t len = end - start;  // (<= 0: no stored element)
    float* v = values + start;

    float kept[CACHE];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < CACHE; ++k) {
        const int64_t j = (int64_t)k * 64 + lane;
        kept[k] = j < len ? v[j] : 0.f;
        acc += (double)kept[k];
    }
#pragma unroll 4
    for (int64_t j = (int64_t)CACHE * 64 + lane; j < len; j += 64) acc += (double)v[j];
    const float s = (float)wave_sum_d(acc);  // (a butterfly: every lane holds the same bits)
    if (lane == 0 && row_sums) row_sums[row] = s;
    if (len <= 0) return;

    const bool dead = s == 0.f;  // stored zeros only
#pragma unroll
    for (int k = 0; k < CACHE; ++k) {
        const int64_t j = (int64_t)k * 64 + lane;
        if (j < len) v[j] = transform(kept[k], target_sum, s, dead);
    }
#pragma unroll 4
    for (int64_t j = (int64_t)CACHE * 64 + lane; j < len; j += 64)
        v[j] = transform(v[j], target_sum, s, dead);
}

template <typename idx_t>
int launch(int64_t n_rows, int64_t nnz, const idx_t* crow, float* values, float target_sum, float* row_sums_out,
           mmvae_stream_t stream) {
    if (n_rows < 1 || n_rows > (int64_t)ROWS * 0x7fffffff || nnz < 0) return MMVAE_ERR_ARG;
    if (!crow || (!values && nnz > 0)) return MMVAE_ERR_ARG;
    if (!isfinite(target_sum) || !(target_sum > 0.f)) return MMVAE_ERR_ARG;
    const unsigned groups = (unsigned)((n_rows + ROWS - 1) / ROWS);
    MMVAE_LAUNCH(csr_log1p_norm_kernel<idx_t>, dim3(groups), dim3(THREADS), 0, (hipStream_t)stream, n_rows, nnz, crow, values,
                 target_sum, row_sums_out);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

}  // namespace

extern "C" int mmvae_prep_abi_version(void) { return MMVAE_PREP_ABI_VERSION; }
extern "C" const char* mmvae_prep_build_arch(void) { return "gfx950"; }

extern "C" int mmvae_prep_csr_log1p_norm_i32(int64_t n_rows, int64_t nnz, const int32_t* crow, float* values,
                                             float target_sum, float* row_sums_out, mmvae_stream_t stream) {
    return launch<int32_t>(n_rows, nnz, crow, values, target_sum, row_sums_out, stream);
}
extern "C" int mmvae_prep_csr_log1p_norm_i64(int64_t n_rows, int64_t nnz, const int64_t* crow, float* values,
                                             float target_sum, float* row_sums_out, mmvae_stream_t stream) {
    return launch<int64_t>(n_rows, nnz, crow, values, target_sum, row_sums_out, stream);
}
