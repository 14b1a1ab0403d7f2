// Per-gene statistics of generated expression matrices (include/mmvae_hip.h, "Per-gene Pearson correlation").
#include "common.h"

namespace {

// Five fp64 moments per column of the values SHIFTED by the column's first row (da = a - a[0][g], db = b - b[0][g]):
// sum da, sum db, sum da^2, sum db^2, sum da db.  The shift is the same for every row chunk, so the chunks' partial
// moments simply add; a constant column's moments are exact zeros, and the mean^2 / variance cancellation of raw moments
// is gone.  A workgroup = 256 columns x one row chunk (lane = 4 adjacent columns, 16-byte loads); wave v takes rows
// v, v + 4, ... of the chunk, four rows of both matrices in flight (clamped, unconditional loads).  Every lane sums its
// rows in row order, the four waves' shares are added in wave order, the chunks in chunk order by the finalising launch:
// no atomics, bitwise reproducible.
constexpr int CP_COLS = 256, CP_MOMENTS = 5, CP_FLIGHT = 4;

// Rows per chunk: the largest power of two in [32, 256] that still gives the grid two workgroups per CU (512), else 32.
// A chunk's partials cost 40 bytes per column to write and 40 to read back, against 8 bytes per row and column of input:
// long chunks keep that share small (8 % at 128 rows), short ones fill the chip when the matrix has few rows.
// Beyond 65 535 chunks (the grid's y extent: millions of rows) the chunks grow instead.
int chunk_rows_for(int B, int G) {
    const long groups = (G + CP_COLS - 1) / CP_COLS;
    int rows = 32;
    for (int r = 256; r > 32; r >>= 1)
        if (groups * ((B + r - 1) / r) >= 512) {
            rows = r;
            break;
        }
    while (((long)B + rows - 1) / rows > 65535) rows <<= 1;
    return rows;
}

__device__ __forceinline__ f32x4 load_group(const float* __restrict__ row, int c, int N, bool whole) {
    if (whole) return *reinterpret_cast<const f32x4*>(row + c);
    f32x4 v;  // element-wise: rows that are not 16-byte groups, the straddling last group (columns clamped into the row)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[min(c + e, N - 1)];
    return v;
}

__global__ __launch_bounds__(256) void col_pearson_moments_kernel(int B, int G, const float* __restrict__ a, int64_t lda,
                                                                  const float* __restrict__ b, int64_t ldb,
                                                                  double* __restrict__ partials, int chunk_rows, int vec) {
    __shared__ double red[3][CP_MOMENTS * 4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * CP_COLS + 4 * lane;
    const int r_begin = blockIdx.y * chunk_rows, r_end = min(r_begin + chunk_rows, B);
    const bool whole = vec && c + 3 < G;
    const int cc = min(c, G - 1);  // (lanes past the last column read it again and store nothing)
    const f32x4 a0 = load_group(a, cc, G, whole), b0 = load_group(b, cc, G, whole);
    double sa[4], sb[4], acc[CP_MOMENTS][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sa[e] = (double)a0[e];
        sb[e] = (double)b0[e];
#pragma unroll
        for (int m = 0; m < CP_MOMENTS; ++m) acc[m][e] = 0.0;
    }
    for (int r0 = r_begin + wave; r0 < r_end; r0 += 4 * CP_FLIGHT) {
        f32x4 va[CP_FLIGHT], vb[CP_FLIGHT];
#pragma unroll
        for (int i = 0; i < CP_FLIGHT; ++i) {
            const int r = min(r0 + 4 * i, r_end - 1);
            va[i] = load_group(a + (int64_t)r * lda, cc, G, whole);
            vb[i] = load_group(b + (int64_t)r * ldb, cc, G, whole);
        }
#pragma unroll
        for (int i = 0; i < CP_FLIGHT; ++i) {
            const bool live = r0 + 4 * i < r_end;  // (a clamped row contributes exact zeros)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double da = live ? (double)va[i][e] - sa[e] : 0.0;
                const double db = live ? (double)vb[i][e] - sb[e] : 0.0;
                acc[0][e] += da;
                acc[1][e] += db;
                acc[2][e] = fma(da, da, acc[2][e]);
                acc[3][e] = fma(db, db, acc[3][e]);
                acc[4][e] = fma(da, db, acc[4][e]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int m = 0; m < CP_MOMENTS; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave - 1][4 * m + e][lane] = acc[m][e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int m = 0; m < CP_MOMENTS; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[m][e] += red[v][4 * m + e][lane];
        double* out = partials + (int64_t)blockIdx.y * CP_MOMENTS * G;  // [chunk][moment][G]
#pragma unroll
        for (int m = 0; m < CP_MOMENTS; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < G) out[(int64_t)m * G + c + e] = acc[m][e];
    }
}

// r[g] from the chunks' moments, added in chunk order.  The three differences are formed the same way, so that a == b
// gives numerator == both variance terms bit for bit and r exactly 1.
__global__ __launch_bounds__(256) void col_pearson_finish_kernel(int B, int G, int chunks, const double* __restrict__ partials,
                                                                 float* __restrict__ r) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double s[CP_MOMENTS];
#pragma unroll
    for (int m = 0; m < CP_MOMENTS; ++m) s[m] = 0.0;
    for (int ch = 0; ch < chunks; ++ch)
#pragma unroll
        for (int m = 0; m < CP_MOMENTS; ++m) s[m] += partials[((int64_t)ch * CP_MOMENTS + m) * G + g];
    const double n = (double)B;
    const double va = fma(n, s[2], -__dmul_rn(s[0], s[0]));
    const double vb = fma(n, s[3], -__dmul_rn(s[1], s[1]));
    const double cov = fma(n, s[4], -__dmul_rn(s[0], s[1]));
    float out = __builtin_nanf("");
    if (va > 0.0 && vb > 0.0) {  // (row 0 shifts to zero: n sum d^2 - (sum d)^2 >= sum d^2 > 0 for a column that varies)
        const double q = cov / sqrt(__dmul_rn(va, vb));
        out = (float)fmin(fmax(q, -1.0), 1.0);
    }
    r[g] = out;
}

}  // namespace

extern "C" size_t mmvae_col_pearson_workspace_bytes(int B, int G) {
    if (B < 2 || G <= 0) return 0;
    const int rows = chunk_rows_for(B, G);
    return (size_t)((B + rows - 1) / rows) * CP_MOMENTS * (size_t)G * sizeof(double);
}

extern "C" int mmvae_col_pearson_f32(int B, int G, const float* a, int64_t lda, const float* b, int64_t ldb, float* r,
                                     void* workspace, size_t workspace_bytes, mmvae_stream_t stream) {
    if (B < 2 || G <= 0 || !a || !b || !r || !workspace || lda < G || ldb < G) return MMVAE_ERR_ARG;
    if (workspace_bytes < mmvae_col_pearson_workspace_bytes(B, G) || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return MMVAE_ERR_ARG;
    const int rows = chunk_rows_for(B, G), chunks = (B + rows - 1) / rows;
    const int vec = aligned16(a) && aligned16(b) && lda % 4 == 0 && ldb % 4 == 0;  // 16-byte row groups in both matrices
    double* partials = static_cast<double*>(workspace);
    MMVAE_LAUNCH(col_pearson_moments_kernel, dim3((G + CP_COLS - 1) / CP_COLS, chunks), dim3(256), 0, (hipStream_t)stream,
                 B, G, a, lda, b, ldb, partials, rows, vec);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(col_pearson_finish_kernel, dim3((G + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, G, chunks,
                 partials, r);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
