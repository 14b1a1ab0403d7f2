// Cell-by-cell correlation of generated expression matrices (include/mmvae_stats.h) -> libmmvae_stats.so.
#include "common.h"
#include "../../include/mmvae_stats.h"

namespace {

constexpr int RB = 128;      // rows per row block (one workgroup multiplies one 128 x 128 pair of blocks)
constexpr int KC = 64;       // genes per staged chunk = length of every fp32 product chain
constexpr int LDS_LD = 66;   // floats per staged row: a 32-lane half of an MFMA operand read (16 rows r, k = 0 / 1) hits
                             // the 32 banks (2 r + k) % 32 once each; rows stay 8-byte aligned for the staging stores
constexpr int GRAM_THREADS = 512;  // 8 waves: 4 (32-row strips) x 2 (64-column halves) of the 128 x 128 tile
constexpr int TILE = RB * RB;
constexpr int ROW_FLIGHT = 4;     // 16-byte groups a thread of the row pass keeps in flight
constexpr int STRIP_ROWS = 256 / RB;        // a finishing workgroup takes 2 rows x 128 columns, one element per thread
constexpr int STRIPS = RB / STRIP_ROWS;     // finishing workgroups per block pair
constexpr int GRAM_TARGET = 256;  // workgroups the gene splits aim at: one per CU (132 KiB of LDS each), none waiting

// The stacked matrix (a ; b), never materialised: row r is row r of a, or row r - n_a of b.
struct Rows {
    const float* a;
    const float* b;
    int64_t lda, ldb;
    int n_a, R, G;
    int vec_a, vec_b;  // 16-byte row groups (base pointer and leading dimension allow it)
};

__device__ __forceinline__ const float* row_of(const Rows& s, int r, int& vec) {
    if (r < s.n_a) {
        vec = s.vec_a;
        return s.a + (int64_t)r * s.lda;
    }
    vec = s.vec_b;
    return s.b + (int64_t)(r - s.n_a) * s.ldb;
}

// x[g .. g + 3] of a row; past the row's end the last element again (the caller masks by g + e < G).
__device__ __forceinline__ f32x4 load_group(const float* __restrict__ row, int g, int G, bool whole) {
    if (whole) return *reinterpret_cast<const f32x4*>(row + g);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[min(g + e, G - 1)];
    return v;
}

// Sum over the 256 threads of a workgroup, the same value in every thread: lanes by butterfly, waves in wave order.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();  // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Workspace: sd [Rpad] fp64, cov_ii [Rpad] fp64, m [Rpad] fp32, constant [Rpad] i32, partial tiles [pairs][splits][128][128] fp64, block sums
// [pairs][STRIPS][3] fp64.
struct Plan {
    int R, nb, pairs, nchunks, splits, cps;
    size_t off_diag, off_m, off_flag, off_tiles, off_sums, bytes;
};

bool make_plan(int n_a, int n_b, int G, Plan& p) {
    if (n_a < 1 || n_b < 0 || G < 2) return false;
    const int64_t R = (int64_t)n_a + n_b;
    if (R < 2 || R > MMVAE_STATS_ROW_CORR_MAX_ROWS) return false;
    p.R = (int)R;
    p.nb = (p.R + RB - 1) / RB;
    p.pairs = p.nb * (p.nb + 1) / 2;
    p.nchunks = (G + KC - 1) / KC;
    int want = GRAM_TARGET / p.pairs;  // R = 200: 3 pairs x 79 .. 85 splits; R = 1024: 36 pairs x 7; R = 2048: 136 pairs x 1
    if (want < 1) want = 1;
    if (want > p.nchunks) want = p.nchunks;
    p.cps = (p.nchunks + want - 1) / want;
    p.splits = (p.nchunks + p.cps - 1) / p.cps;  // (no empty split)
    const size_t rpad = (size_t)p.nb * RB;
    p.off_diag = rpad * sizeof(double);
    p.off_m = p.off_diag + rpad * sizeof(double);
    p.off_flag = p.off_m + rpad * sizeof(float);
    p.off_tiles = p.off_flag + rpad * sizeof(int);
    p.off_sums = p.off_tiles + (size_t)p.pairs * p.splits * TILE * sizeof(double);
    p.bytes = p.off_sums + (size_t)p.pairs * STRIPS * 3 * sizeof(double);
    return true;
}

// (bi, bj), bi <= bj, of upper-triangular pair p; pair_of is its inverse.
__device__ __forceinline__ void pair_blocks(int p, int nb, int& bi, int& bj) {
    bi = 0;
    while (p >= nb - bi) {
        p -= nb - bi;
        ++bi;
    }
    bj = bi + p;
}
__device__ __forceinline__ int pair_of(int bi, int bj, int nb) { return bi * nb - bi * (bi - 1) / 2 + (bj - bi); }

// ---------------------------------------------------------------------------------------------------- 1. row pass
// One workgroup per row.  Thread t takes the 4-element groups t, t + 256, ... whichever load form the row allows, so
// the summation order -- and with it every bit of m and sd -- does not depend on alignment or on which operand holds
// the row.  The second sweep (the row is cache-resident by then) adds the centred fp32 values the Gram pass will
// multiply, d = fl32(x_ig - m_i): sd_i = sum_g d and sum_g d^2, in fp64, and from them the row's own
// cov_ii = sum d^2 - sd_i^2 / G -- the diagonal every r_ij divides by is complete, and carries no fp32 chain error,
// before the Gram pass starts.
__global__ __launch_bounds__(256) void row_corr_rows_kernel(Rows s, double* __restrict__ sd, double* __restrict__ diag,
                                                            float* __restrict__ m, int* __restrict__ constant) {
    __shared__ double red[4];
    const int r = blockIdx.x, G = s.G;
    int vec;
    const float* __restrict__ row = row_of(s, r, vec);
    const float x0 = row[0];
    const double x0d = (double)x0;
    double sum = 0.0;
    int varies = 0;
    for (int g0 = 4 * threadIdx.x; g0 < G; g0 += 1024 * ROW_FLIGHT) {
        f32x4 v[ROW_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROW_FLIGHT; ++u) {
            const int g = g0 + 1024 * u;
            v[u] = load_group(row, min(g, G - 1), G, vec && g + 3 < G);
        }
#pragma unroll
        for (int u = 0; u < ROW_FLIGHT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (g0 + 1024 * u + e < G) {
                    sum += (double)v[u][e] - x0d;
                    varies |= v[u][e] != x0;
                }
    }
    sum = block_sum_d(sum, red);
    varies = __syncthreads_or(varies);
    const float mean = (float)(x0d + sum / (double)G);
    double res = 0.0, sq = 0.0;
    for (int g0 = 4 * threadIdx.x; g0 < G; g0 += 1024 * ROW_FLIGHT) {
        f32x4 v[ROW_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROW_FLIGHT; ++u) {
            const int g = g0 + 1024 * u;
            v[u] = load_group(row, min(g, G - 1), G, vec && g + 3 < G);
        }
#pragma unroll
        for (int u = 0; u < ROW_FLIGHT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (g0 + 1024 * u + e < G) {
                    const double d = (double)(v[u][e] - mean);
                    res += d;
                    sq = fma(d, d, sq);
                }
    }
    res = block_sum_d(res, red);
    sq = block_sum_d(sq, red);
    if (threadIdx.x == 0) {
        sd[r] = res;
        diag[r] = sq - __dmul_rn(res, res) / (double)G;
        m[r] = mean;
        constant[r] = !varies;
    }
}

// --------------------------------------------------------------------------------------------------- 2. Gram pass
// Workgroup (pair of row blocks, gene split): S[i][j] = sum_g d_ig d_jg over the split's genes, d = x - m_i in fp32 and
// exact zeros past G and past R.  Thread t stages genes 4 (t & 15) .. + 3 of rows (t >> 4) + 32 i of both blocks; wave w
// multiplies rows 32 (w >> 1) .. + 31 of block bi with rows 64 (w & 1) .. + 63 of block bj: eight independent 16 x 16
// accumulators, 16 k-steps of v_mfma_f32_16x16x4_f32 per chunk = one 64-gene fmaf chain each, then flushed into fp64.
// The next chunk's global loads are issued ahead of the products and land in the other LDS buffer behind them: one
// barrier per chunk.  A 128 x 128 tile reads 256 rows for 16 384 products per gene: half the operand traffic per
// product of a 64 x 64 tile, which is what bounds this pass at R >= 1024.
struct Staged {
    f32x4 v[4];
};

// The raw values only: nothing here consumes a loaded register, so the loads stay in flight behind the products.
__device__ __forceinline__ void stage_load(const Rows& s, int block, int chunk, Staged& out) {
    const int g = chunk * KC + 4 * (threadIdx.x & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = block * RB + (threadIdx.x >> 4) + 32 * i;
        int vec;
        const float* __restrict__ row = row_of(s, r < s.R ? r : 0, vec);
        out.v[i] = load_group(row, min(g, s.G - 1), s.G, vec && g + 3 < s.G);
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Centre and store: d = x - m_i in fp32; columns past G and rows past R are exact zeros (not 0 - m_i).
__device__ __forceinline__ void stage_store(float* __restrict__ lds, const Rows& s, int block, int chunk,
                                            const float (&mean)[4], const Staged& in) {
    const int g = chunk * KC + 4 * (threadIdx.x & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool live = block * RB + (threadIdx.x >> 4) + 32 * i < s.R;
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = (live && g + e < s.G) ? in.v[i][e] - mean[i] : 0.f;
        float* __restrict__ dst = lds + ((threadIdx.x >> 4) + 32 * i) * LDS_LD + 4 * (threadIdx.x & 15);
        *reinterpret_cast<f32x2*>(dst) = f32x2{d[0], d[1]};
        *reinterpret_cast<f32x2*>(dst + 2) = f32x2{d[2], d[3]};
    }
}

__global__ __launch_bounds__(GRAM_THREADS) void row_corr_gram_kernel(Rows s, const float* __restrict__ m,
                                                                     double* __restrict__ tiles, int nb, int nchunks,
                                                                     int splits, int cps) {
    __shared__ __attribute__((aligned(16))) float lds[2][2][RB * LDS_LD];
    const int pair = blockIdx.x / splits, split = blockIdx.x % splits;
    int bi, bj;
    pair_blocks(pair, nb, bi, bj);
    const bool same = bi == bj;
    const int c_begin = split * cps, c_end = min(c_begin + cps, nchunks);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;

    float mean_a[4], mean_b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = bi * RB + (threadIdx.x >> 4) + 32 * i, rb = bj * RB + (threadIdx.x >> 4) + 32 * i;
        mean_a[i] = ra < s.R ? m[ra] : 0.f;
        mean_b[i] = rb < s.R ? m[rb] : 0.f;
    }
    Staged pa, pb;
    stage_load(s, bi, c_begin, pa);
    if (!same) stage_load(s, bj, c_begin, pb);
    stage_store(lds[0][0], s, bi, c_begin, mean_a, pa);
    if (!same) stage_store(lds[0][1], s, bj, c_begin, mean_b, pb);
    __syncthreads();

    double acc64[2][4][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc64[a][n][e] = 0.0;

    for (int c = c_begin; c < c_end; ++c) {
        const int buf = (c - c_begin) & 1;
        const bool more = c + 1 < c_end;
        if (more) {
            stage_load(s, bi, c + 1, pa);
            if (!same) stage_load(s, bj, c + 1, pb);
        }
        const float* __restrict__ A = lds[buf][0] + (32 * wr + (lane & 15)) * LDS_LD + (lane >> 4);
        const float* __restrict__ B = lds[buf][same ? 0 : 1] + (64 * wc + (lane & 15)) * LDS_LD + (lane >> 4);
        f32x4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[a][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            float av[2], bv[4];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = A[16 * a * LDS_LD + 4 * kk];
#pragma unroll
            for (int n = 0; n < 4; ++n) bv[n] = B[16 * n * LDS_LD + 4 * kk];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[a][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[n], acc[a][n], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc64[a][n][e] += (double)acc[a][n][e];
        if (more) {
            stage_store(lds[buf ^ 1][0], s, bi, c + 1, mean_a, pa);
            if (!same) stage_store(lds[buf ^ 1][1], s, bj, c + 1, mean_b, pb);
        }
        __syncthreads();
    }
    // accumulator element e of tile (a, n): row 32 wr + 16 a + 4 (lane >> 4) + e of block bi, column 64 wc + 16 n +
    // (lane & 15) of block bj
    double* __restrict__ out = tiles + (int64_t)blockIdx.x * TILE;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                out[(32 * wr + 16 * a + 4 * (lane >> 4) + e) * RB + 64 * wc + 16 * n + (lane & 15)] = acc64[a][n][e];
}

// ------------------------------------------------------------------------------------------------------ 3. finish
// One workgroup per (block pair, strip of 2 rows), one element per thread: the splits' partial sums added in split
// order, cov_ij = S_ij - sd_i sd_j / G, r_ij = cov_ij / sqrt(cov_ii cov_jj) for the upper-triangular elements, stored and
// mirrored; then the workgroup's share of the three block sums (cis, cross, comb) in a fixed order: butterfly, wave order.
__global__ __launch_bounds__(256) void row_corr_finish_kernel(int n_a, int R, int G, int nb, int splits,
                                                              const double* __restrict__ sd,
                                                              const double* __restrict__ diag,
                                                              const int* __restrict__ constant,
                                                              const double* __restrict__ tiles, float* __restrict__ corr,
                                                              int64_t ldc, double* __restrict__ sums) {
    __shared__ double red[4];
    const int pair = blockIdx.x / STRIPS, strip = blockIdx.x % STRIPS, t = threadIdx.x;
    int bi, bj;
    pair_blocks(pair, nb, bi, bj);
    const int ri = STRIP_ROWS * strip + t / RB, cj = t % RB, i = bi * RB + ri, j = bj * RB + cj, e = ri * RB + cj;
    double s_cis = 0.0, s_cross = 0.0, s_comb = 0.0;
    if (i < R && j < R && i <= j) {
        const double* __restrict__ src = tiles + (int64_t)pair * splits * TILE + e;
        double S = 0.0;
#pragma unroll 16
        for (int sp = 0; sp < splits; ++sp) S += src[(int64_t)sp * TILE];
        const double cov = S - __dmul_rn(sd[i], sd[j]) / (double)G;
        double q = cov / sqrt(__dmul_rn(diag[i], diag[j]));
        q = q > 1.0 ? 1.0 : (q < -1.0 ? -1.0 : q);  // (keeps a NaN)
        const bool dead = constant[i] | constant[j];
        if (i == j) q = 1.0;
        if (corr) {
            const float out = dead ? __builtin_nanf("") : (float)q;
            corr[(int64_t)i * ldc + j] = out;
            corr[(int64_t)j * ldc + i] = out;
        }
        if (dead || q != q) q = 0.0;  // nan_to_num
        const double both = i == j ? q : 2.0 * q;  // (i, j) and its mirror image lie in the same square block
        if (j < n_a) s_cis = both;
        else if (i >= n_a) s_cross = both;
        else s_comb = q;
    }
    s_cis = block_sum_d(s_cis, red);
    s_cross = block_sum_d(s_cross, red);
    s_comb = block_sum_d(s_comb, red);
    if (t == 0) {
        sums[3 * blockIdx.x + 0] = s_cis;
        sums[3 * blockIdx.x + 1] = s_cross;
        sums[3 * blockIdx.x + 2] = s_comb;
    }
}

// One workgroup: thread t adds partial sums t, t + 256, ... in order, then butterfly and wave order.
__global__ __launch_bounds__(256) void row_corr_stats_kernel(int n_a, int R, int parts, const double* __restrict__ sums,
                                                             const int* __restrict__ constant, double* __restrict__ stats) {
    __shared__ double red[4];
    double s[3] = {0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < parts; p += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += sums[3 * p + k];
    double dead_a = 0.0, dead_b = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) {
        if (r < n_a) dead_a += (double)constant[r];
        else dead_b += (double)constant[r];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = block_sum_d(s[k], red);
    dead_a = block_sum_d(dead_a, red);
    dead_b = block_sum_d(dead_b, red);
    if (threadIdx.x == 0) {
        const double na = (double)n_a, nbr = (double)(R - n_a);
        const double cis = s[0] / (na * na), cross = s[1] / (nbr * nbr), comb = s[2] / (na * nbr);  // n_b == 0: 0 / 0
        stats[0] = cis;
        stats[1] = cross;
        stats[2] = comb;
        stats[3] = 2.0 * comb / (cis + cross);
        stats[4] = dead_a;
        stats[5] = dead_b;
        stats[6] = 0.0;
        stats[7] = 0.0;
    }
}

}  // namespace

extern "C" int mmvae_stats_abi_version(void) { return MMVAE_STATS_ABI_VERSION; }
extern "C" const char* mmvae_stats_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_stats_row_corr_workspace_bytes(int n_a, int n_b, int G) {
    Plan p;
    return make_plan(n_a, n_b, G, p) ? p.bytes : 0;
}

extern "C" int mmvae_stats_row_corr_f32(int n_a, int n_b, int G, const float* a, int64_t lda, const float* b, int64_t ldb,
                                        float* corr, int64_t ldc, double* stats, void* workspace, size_t workspace_bytes,
                                        mmvae_stream_t stream) {
    Plan p;
    if (!make_plan(n_a, n_b, G, p)) return MMVAE_ERR_ARG;
    if (!a || lda < G || !stats || !workspace || (b == nullptr) != (n_b == 0) || (b && ldb < G)) return MMVAE_ERR_ARG;
    if (corr && ldc < p.R) return MMVAE_ERR_ARG;
    if (workspace_bytes < p.bytes || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return MMVAE_ERR_ARG;
    char* ws = static_cast<char*>(workspace);
    double* sd = reinterpret_cast<double*>(ws);
    double* diag = reinterpret_cast<double*>(ws + p.off_diag);
    float* m = reinterpret_cast<float*>(ws + p.off_m);
    int* constant = reinterpret_cast<int*>(ws + p.off_flag);
    double* tiles = reinterpret_cast<double*>(ws + p.off_tiles);
    double* sums = reinterpret_cast<double*>(ws + p.off_sums);
    Rows s;
    s.a = a;
    s.b = b ? b : a;
    s.lda = lda;
    s.ldb = b ? ldb : lda;
    s.n_a = n_a;
    s.R = p.R;
    s.G = G;
    s.vec_a = aligned16(a) && lda % 4 == 0;
    s.vec_b = b ? (aligned16(b) && ldb % 4 == 0) : s.vec_a;
    hipStream_t st = (hipStream_t)stream;
    MMVAE_LAUNCH(row_corr_rows_kernel, dim3(p.R), dim3(256), 0, st, s, sd, diag, m, constant);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(row_corr_gram_kernel, dim3(p.pairs * p.splits), dim3(GRAM_THREADS), 0, st, s, (const float*)m, tiles, p.nb,
                 p.nchunks, p.splits, p.cps);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(row_corr_finish_kernel, dim3(p.pairs * STRIPS), dim3(256), 0, st, n_a, p.R, G, p.nb, p.splits, (const double*)sd,
                 (const double*)diag, (const int*)constant, (const double*)tiles, corr, ldc, sums);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(row_corr_stats_kernel, dim3(1), dim3(256), 0, st, n_a, p.R, p.pairs * STRIPS, (const double*)sums,
                 (const int*)constant, stats);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
