// K-means on latent embeddings (include/mmvae_clust.h) -> libmmvae_clust.so.
//
// The Lloyd step walks the exact-fp32 MFMA Gram tiles of knn_gram_kernel (umap_knn.hip) and sil_gram_kernel
// (sil_rows.hip): 64 rows of x to a workgroup, 16 to a wave as the A operands of v_mfma_f32_16x16x4_f32, the padded
// centroids as column tiles of 64 through a double-buffered LDS chunk.  The staging code is repeated here on purpose (the
// other two files are left as they are).  What differs: the rows are read straight from x (bounds-checked, no padded
// image: x is read from HBM once), a workgroup walks a RANGE of row tiles, and after a tile's labels are known the tile
// is read a second time (from the L2) and summed, cluster by cluster, into the workgroup's own fp64 [C, D] sums.
#include "common.h"
#include "../../include/mmvae_clust.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int BM = 16 * WAVES;  // rows of x per tile: 16 to a wave
constexpr int BN = 64;          // centroids per column tile
constexpr int KC = 64;          // columns per staged chunk
constexpr int LDB = KC + 2;     // floats per staged row (bank layout: see umap_knn.hip)
constexpr int MAX_GRID = 512;
constexpr size_t PARTIAL_BUDGET = (size_t)64 << 20;  // bytes of fp64 [C, D] sums over the whole grid

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Stats {
    double inertia;
    double shift2;
    int32_t changed;
    int32_t empty;
};
static_assert(sizeof(Stats) == MMVAE_CLUST_STATS_BYTES, "the stats record of mmvae_clust.h");

inline int padded_d(int D) { return D <= 64 ? 64 : D <= 128 ? 128 : D <= 256 ? 256 : 512; }
inline int padded_c(int C) { return (C + BN - 1) / BN * BN; }
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
bool shape_ok(int N, int D, int C) {
    return N >= 1 && D >= 1 && D <= MMVAE_CLUST_MAX_D && C >= 1 && C <= MMVAE_CLUST_MAX_C && C <= N;
}

// The grid of the assignment pass, a function of the shape alone: at most MAX_GRID workgroups, fewer while their fp64
// sums exceed PARTIAL_BUDGET; every workgroup gets `per` consecutive row tiles (the last one what is left).
struct Grid {
    int tiles, per, groups;
};
Grid grid_of(int N, int D, int C) {
    Grid g;
    g.tiles = (int)(((int64_t)N + BM - 1) / BM);
    int64_t cap = (int64_t)(PARTIAL_BUDGET / ((size_t)C * D * sizeof(double)));
    if (cap < 1) cap = 1;
    int want = g.tiles < MAX_GRID ? g.tiles : MAX_GRID;
    if (want > cap) want = (int)cap;
    g.per = (g.tiles + want - 1) / want;
    g.groups = (g.tiles + g.per - 1) / g.per;
    return g;
}

struct Workspace {
    size_t cp, cnorm, part, pcount, pinertia, pchanged, shiftc, bytes;
};
Workspace layout(int N, int D, int C) {
    const Grid g = grid_of(N, D, C);
    const size_t CP = padded_c(C), DP = padded_d(D), G = g.groups;
    Workspace w;
    size_t at = 0;
    w.cp = at, at += up16(CP * DP * sizeof(float));
    w.cnorm = at, at += up16(CP * sizeof(float));
    w.part = at, at += up16(G * C * D * sizeof(double));
    w.pcount = at, at += up16(G * C * sizeof(int32_t));
    w.pinertia = at, at += up16(G * sizeof(double));
    w.pchanged = at, at += up16(G * sizeof(int32_t));
    w.shiftc = at, at += up16((size_t)C * sizeof(double));
    w.bytes = at;
    return w;
}

// ------------------------------------------------------------------------------------------------ 1. the centroids
// One workgroup per 16 rows of the padded [CP, DP] image: every wave writes four rows (lane l the columns l, l + 64, ...;
// rows past C and columns past D are exact zeros), and wave 0 takes the 16 squared norms m_c = g(c, c) from the diagonal
// of the Gram pass's own MFMA chain over DP, reading the centroids themselves.
__global__ __launch_bounds__(THREADS) void clust_centroids_kernel(int C, int D, int DP, const float* __restrict__ cen,
                                                                  float* __restrict__ cp, float* __restrict__ cnorm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * 16;
    for (int j = 0; j < 4; ++j) {
        const int r = row0 + 4 * wave + j;
        for (int c = lane; c < DP; c += 64) cp[(int64_t)r * DP + c] = (r < C && c < D) ? cen[(int64_t)r * D + c] : 0.f;
    }
    if (wave == 0) {
        const int r = row0 + (lane & 15), q = lane >> 4;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < DP / 4; ++kk) {
            const int k = 4 * kk + q;
            const float v = (r < C && k < D) ? cen[(int64_t)r * D + k] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v, v, acc, 0, 0, 0);
        }
        // accumulator element e: row 4 (lane >> 4) + e, column lane & 15
        const int e = (lane & 15) - 4 * q;
        if (e >= 0 && e < 4) cnorm[r] = e == 0 ? acc[0] : e == 1 ? acc[1] : e == 2 ? acc[2] : acc[3];
    }
}

// ------------------------------------------------------------------------------------------------ 2. assign + sums
constexpr int STAGE_V = BN * KC / 4 / THREADS;  // 16-byte groups of a 64 x 64 chunk per thread
struct StagedB {
    f32x4 v[STAGE_V];
};

template <int DP>
__device__ __forceinline__ void stage_load(const float* __restrict__ cp, int tile, int chunk, StagedB& out) {
#pragma unroll
    for (int v = 0; v < STAGE_V; ++v) {
        const int q = threadIdx.x + v * THREADS;
        out.v[v] = *reinterpret_cast<const f32x4*>(cp + ((int64_t)tile * BN + (q >> 4)) * DP + chunk * KC + 4 * (q & 15));
    }
}
__device__ __forceinline__ void stage_store(float* __restrict__ lds, const StagedB& in) {
#pragma unroll
    for (int v = 0; v < STAGE_V; ++v) {
        const int q = threadIdx.x + v * THREADS;
        float* __restrict__ dst = lds + (q >> 4) * LDB + 4 * (q & 15);
        *reinterpret_cast<f32x2*>(dst) = f32x2{in.v[v][0], in.v[v][1]};
        *reinterpret_cast<f32x2*>(dst + 2) = f32x2{in.v[v][2], in.v[v][3]};
    }
}

// Workgroup b owns the row tiles [b per, min(tiles, (b + 1) per)) and row b of every per-workgroup table.  Per tile:
//
//   scores   wave w holds rows 16 w .. + 15 of the tile as A operands (lane l: row l & 15, k = 4 kk + (l >> 4)); n_i is
//            the diagonal of the rows' own Gram block.  Over the centroid tiles, accumulator element e of block n is
//            g(row 4 (l >> 4) + e, centroid 64 ct + 16 n + (l & 15)); a lane keeps the best of its centroids in ascending
//            order (strict <), and the 16 lanes of a DPP row settle the row's minimum by (d2, index).
//   order    wave 0 ranks the tile's rows by (label, row) and lists where every cluster's rows begin; lane 0 of wave 1
//            adds the tile's dist2 to the workgroup's inertia, row after row.
//   sums     thread (column d mod W, cluster c mod 256 / W) adds, for each of its clusters present in the tile, the rows
//            in ascending order in fp32 and that sum to its fp64 cell (c, d).  A cell has one owner for the whole call.
template <int DP>
__global__ __launch_bounds__(THREADS) void clust_assign_kernel(int N, int D, const float* __restrict__ x, int64_t ldx, int C,
                                                               int n_ctiles, const float* __restrict__ cp,
                                                               const float* __restrict__ cnorm, int32_t* label,
                                                               float* __restrict__ dist2, double* part, int32_t* pcount,
                                                               double* __restrict__ pinertia, int32_t* __restrict__ pchanged,
                                                               int tiles, int per) {
    constexpr int NCH = DP / KC;
    constexpr int W = DP < THREADS ? DP : THREADS;  // threads across the columns in the summing phase
    constexpr int GROUPS = THREADS / W;             // ... and across the clusters
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * LDB];
    __shared__ int s_label[BM], s_sorted[BM], s_order[BM], s_seg[BM + 1], s_nseg, s_changed[WAVES];
    __shared__ float s_d2[BM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane & 15, q = lane >> 4;
    const int col = threadIdx.x % W, grp = threadIdx.x / W;
    const int t_begin = blockIdx.x * per, t_end = min(tiles, t_begin + per);

    double* mypart = part + (int64_t)blockIdx.x * C * D;
    int32_t* mycount = pcount + (int64_t)blockIdx.x * C;
    for (int c = grp; c < C; c += GROUPS) {
        for (int d = col; d < D; d += W) mypart[(int64_t)c * D + d] = 0.0;
        if (col == 0) mycount[c] = 0;
    }
    double inertia = 0.0;  // (thread 64's)
    int changed = 0;

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t tile_row0 = (int64_t)tile * BM;
        const int nv = (int)min((int64_t)BM, (int64_t)N - tile_row0);  // rows of this tile
        float areg[DP / 4];
        {
            // (a row past N reads row 0 instead: it is an ordinary row whose results are never stored)
            const int64_t r = tile_row0 + 16 * wave + cl;
            const float* __restrict__ arow = x + (r < N ? r : 0) * ldx + q;
            if (D == DP) {
#pragma unroll
                for (int kk = 0; kk < DP / 4; ++kk) areg[kk] = arow[4 * kk];
            } else {
#pragma unroll
                for (int kk = 0; kk < DP / 4; ++kk) areg[kk] = 4 * kk + q < D ? arow[4 * kk] : 0.f;
            }
        }
        int old[4] = {0, 0, 0, 0};  // the labels read, asked for now and used behind the centroid loop
        if (cl == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t row = tile_row0 + 16 * wave + 4 * q + e;
                if (row < N) old[e] = label[row];
            }
        }
        float ni[4];
        {
            f32x4 nacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < DP / 4; ++kk) nacc = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[kk], areg[kk], nacc, 0, 0, 0);
            // element e of lane (q, cl) is g(row 4 q + e, row cl): the diagonal of row 4 q + e sits in lane cl = 4 q + e
#pragma unroll
            for (int e = 0; e < 4; ++e) ni[e] = __shfl(nacc[e], (lane & 48) + 4 * q + e, 64);
        }
        float bd[4];
        int bi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bd[e] = __builtin_inff();
            bi[e] = 0x7fffffff;
        }

        StagedB p;
        stage_load<DP>(cp, 0, 0, p);
        stage_store(Bs[0], p);
        __syncthreads();
        for (int ct = 0; ct < n_ctiles; ++ct) {
            f32x4 acc[4];
            float mc[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                mc[n] = cnorm[ct * BN + 16 * n + cl];
            }
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int buf = (ct * NCH + ch) & 1;
                const bool last_chunk = ch == NCH - 1;
                const bool more = !(last_chunk && ct + 1 == n_ctiles);
                if (more) stage_load<DP>(cp, last_chunk ? ct + 1 : ct, last_chunk ? 0 : ch + 1, p);
                const float* __restrict__ B = Bs[buf] + cl * LDB + q;
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
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const int c = ct * BN + 16 * n + cl;
                        if (c < C) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float v = fmaxf((ni[e] + mc[n]) - 2.f * acc[n][e], 0.f);
                                if (v < bd[e]) {
                                    bd[e] = v;
                                    bi[e] = c;
                                }
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        // the row's minimum over the 16 lanes that hold its centroids: (d2, index) in lexicographic order
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                const float od = __shfl_xor(bd[e], m, 64);
                const int oi = __shfl_xor(bi[e], m, 64);
                if (od < bd[e] || (od == bd[e] && oi < bi[e])) {
                    bd[e] = od;
                    bi[e] = oi;
                }
            }
        }
        if (cl == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int rt = 16 * wave + 4 * q + e;
                const int64_t row = tile_row0 + rt;
                const bool live = row < N;
                const bool found = bi[e] < C;  // (not found: every score was +inf; cluster 0 then)
                const int lab = found ? bi[e] : 0;
                const float d = found ? bd[e] : 0.f;
                s_label[rt] = live ? lab : 0x7fffffff;
                s_d2[rt] = live ? d : 0.f;
                if (live) {
                    changed += old[e] != lab;
                    label[row] = lab;
                    dist2[row] = d;
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int mine = s_label[lane];
            int rank = 0;  // (a row past N has the largest label: it is counted by no row in front of it)
#pragma unroll 16
            for (int r = 0; r < BM; ++r) {
                const int l = s_label[r];
                rank += (l < mine) || (l == mine && r < lane);
            }
            if (lane < nv) {
                s_order[rank] = lane;
                s_sorted[rank] = mine;
            }
        } else if (threadIdx.x == 64) {
#pragma unroll 16
            for (int r = 0; r < BM; ++r) inertia += (double)s_d2[r];  // (a row past N holds 0)
        }
        __syncthreads();
        if (wave == 0) {
            const bool start = lane < nv && (lane == 0 || s_sorted[lane] != s_sorted[lane - 1]);
            const unsigned long long mask = __ballot(start);
            if (start) s_seg[__popcll(mask & ((1ull << lane) - 1ull))] = lane;
            if (lane == 0) {
                const int nseg = __popcll(mask);
                s_seg[nseg] = nv;
                s_nseg = nseg;
            }
        }
        __syncthreads();
        {
            // Eight clusters of the tile at a time, so that the loads of their first rows, and then of their fp64 cells, are
            // in flight together (the cells of one batch are distinct); a cluster's sum starts with its first row, the
            // others follow in ascending order, eight loads at a time.
            constexpr int SB = 8;
            const int nseg = s_nseg;
            for (int d = col; d < D; d += W) {
                const float* __restrict__ xd = x + tile_row0 * ldx + d;
                for (int s0 = 0; s0 < nseg; s0 += SB) {
                    float v[SB];
                    int cell[SB];
#pragma unroll
                    for (int j = 0; j < SB; ++j) {
                        const int s = s0 + j;
                        cell[j] = -1;
                        v[j] = 0.f;
                        if (s < nseg) {
                            const int p0 = s_seg[s], p1 = s_seg[s + 1];
                            const int c = s_sorted[p0];
                            if (c % GROUPS == grp) {
                                cell[j] = c * D + d;
                                v[j] = xd[s_order[p0] * ldx];
                                int pp = p0 + 1;
                                for (; pp + 8 <= p1; pp += 8) {
                                    float t[8];
#pragma unroll
                                    for (int i = 0; i < 8; ++i) t[i] = xd[s_order[pp + i] * ldx];
#pragma unroll
                                    for (int i = 0; i < 8; ++i) v[j] += t[i];
                                }
                                if (pp + 4 <= p1) {
                                    float t[4];
#pragma unroll
                                    for (int i = 0; i < 4; ++i) t[i] = xd[s_order[pp + i] * ldx];
#pragma unroll
                                    for (int i = 0; i < 4; ++i) v[j] += t[i];
                                    pp += 4;
                                }
                                for (; pp < p1; ++pp) v[j] += xd[s_order[pp] * ldx];
                            }
                        }
                    }
                    double a[SB];
#pragma unroll
                    for (int j = 0; j < SB; ++j)
                        if (cell[j] >= 0) a[j] = mypart[cell[j]];
#pragma unroll
                    for (int j = 0; j < SB; ++j)
                        if (cell[j] >= 0) mypart[cell[j]] = a[j] + (double)v[j];
                }
            }
            if (col == 0) {
                for (int s = 0; s < nseg; ++s) {
                    const int p0 = s_seg[s], p1 = s_seg[s + 1];
                    const int c = s_sorted[p0];
                    if (c % GROUPS == grp) mycount[c] += p1 - p0;
                }
            }
        }
        // (the next tile writes s_label, s_order, s_sorted and s_seg only behind the barriers of its centroid loop)
    }
    if (threadIdx.x == 64) pinertia[blockIdx.x] = inertia;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) changed += __shfl_xor(changed, m, 64);
    if (lane == 0) s_changed[wave] = changed;
    __syncthreads();
    if (threadIdx.x == 0) pchanged[blockIdx.x] = s_changed[0] + s_changed[1] + s_changed[2] + s_changed[3];
}

// ------------------------------------------------------------------------------------------------ 3. the means
// One workgroup per cluster: the workgroups' sums in ascending order, the mean, and the cluster's share of shift2.
__global__ __launch_bounds__(THREADS) void clust_means_kernel(int D, int C, int G, const float* __restrict__ cen,
                                                              const double* __restrict__ part,
                                                              const int32_t* __restrict__ pcount, float* __restrict__ out,
                                                              int32_t* __restrict__ counts, double* __restrict__ shiftc) {
    __shared__ double red[THREADS];
    const int c = blockIdx.x;
    int cnt = 0;
#pragma unroll 16
    for (int g = 0; g < G; ++g) cnt += pcount[(int64_t)g * C + c];
    double sh = 0.0;
    for (int d = threadIdx.x; d < D; d += THREADS) {
        // (sixteen loads in flight at a time; the additions stay in ascending order)
        const double* __restrict__ p = part + (int64_t)c * D + d;
        const int64_t step = (int64_t)C * D;
        double s = 0.0;
        int g = 0;
        for (; g + 16 <= G; g += 16) {
            double t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) t[j] = p[(g + j) * step];
#pragma unroll
            for (int j = 0; j < 16; ++j) s += t[j];
        }
        for (; g < G; ++g) s += p[g * step];
        const float old = cen[(int64_t)c * D + d];
        const float nw = cnt > 0 ? (float)(s / (double)cnt) : old;
        out[(int64_t)c * D + d] = nw;
        const double diff = (double)nw - (double)old;
        sh += diff * diff;
    }
    red[threadIdx.x] = sh;
    __syncthreads();
    for (int stride = THREADS / 2; stride >= 1; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        shiftc[c] = red[0];
        counts[c] = cnt;
    }
}

// ------------------------------------------------------------------------------------------------ 4. the record
__global__ void clust_stats_kernel(int C, int G, const double* __restrict__ pinertia, const int32_t* __restrict__ pchanged,
                                   const double* __restrict__ shiftc, const int32_t* __restrict__ counts,
                                   Stats* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double inertia = 0.0, shift2 = 0.0;
    int changed = 0, empty = 0;
    for (int g = 0; g < G; ++g) {
        inertia += pinertia[g];
        changed += pchanged[g];
    }
    for (int c = 0; c < C; ++c) {
        shift2 += shiftc[c];
        empty += counts[c] == 0;
    }
    stats->inertia = inertia;
    stats->shift2 = shift2;
    stats->changed = changed;
    stats->empty = empty;
}

template <int DP>
int launch_assign(const Grid& g, int N, int D, const float* x, int64_t ldx, int C, const float* cp, const float* cnorm,
                  int32_t* label, float* dist2, double* part, int32_t* pcount, double* pinertia, int32_t* pchanged,
                  hipStream_t st) {
    MMVAE_LAUNCH((clust_assign_kernel<DP>), dim3((unsigned)g.groups), dim3(THREADS), 0, st, N, D, x, ldx, C, padded_c(C) / BN,
                 cp, cnorm, label, dist2, part, pcount, pinertia, pchanged, g.tiles, g.per);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

// ------------------------------------------------------------------------------------------------ seeding
// A wave owns 64 rows.  Per chunk of 64 columns it reads them row by row (lane = column: whole lines) into its own
// [64][65] LDS square, and lane r then walks row r of the square: the chain of row r runs over d in ascending order.
__global__ __launch_bounds__(THREADS) void clust_seed_kernel(int N, int D, const float* __restrict__ x, int64_t ldx, int row,
                                                             int first, float* __restrict__ mind2) {
    __shared__ float T[WAVES][64 * 65];
    __shared__ float xr[MMVAE_CLUST_MAX_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < D; d += THREADS) xr[d] = x[(int64_t)row * ldx + d];
    const int64_t r0 = ((int64_t)blockIdx.x * WAVES + wave) * 64;
    float* __restrict__ mine = T[wave];
    float acc = 0.f;
    for (int k0 = 0; k0 < D; k0 += 64) {
        const int kc = min(64, D - k0);
        __syncthreads();
        for (int j = 0; j < 64; ++j) {
            const int64_t r = r0 + j;
            mine[j * 65 + lane] = (lane < kc && r < N) ? x[r * ldx + k0 + lane] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            const float diff = mine[lane * 65 + k] - xr[k0 + k];
            acc = fmaf(diff, diff, acc);
        }
    }
    const int64_t i = r0 + lane;
    if (i < N) mind2[i] = first ? acc : fminf(mind2[i], acc);
}

}  // namespace

extern "C" int mmvae_clust_abi_version(void) { return MMVAE_CLUST_ABI_VERSION; }
extern "C" const char* mmvae_clust_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_clust_kmeans_workspace_bytes(int N, int D, int C) {
    if (!shape_ok(N, D, C)) return 0;
    return layout(N, D, C).bytes;
}

extern "C" int mmvae_clust_kmeans_step_f32(int N, int D, const float* x, int64_t ldx, int C, const float* centroids,
                                           float* new_centroids, int32_t* label, float* dist2, int32_t* counts, void* stats,
                                           void* workspace, size_t workspace_bytes, mmvae_stream_t stream) {
    if (!shape_ok(N, D, C) || ldx < D) return MMVAE_ERR_ARG;
    if (!x || !centroids || !new_centroids || !label || !dist2 || !counts || !stats || !workspace) return MMVAE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(stats) & 7u) != 0) return MMVAE_ERR_ARG;
    const Workspace w = layout(N, D, C);
    if (workspace_bytes < w.bytes || !aligned16(workspace)) return MMVAE_ERR_ARG;
    const Grid g = grid_of(N, D, C);
    const int DP = padded_d(D), CP = padded_c(C);
    char* base = static_cast<char*>(workspace);
    float* cp = reinterpret_cast<float*>(base + w.cp);
    float* cnorm = reinterpret_cast<float*>(base + w.cnorm);
    double* part = reinterpret_cast<double*>(base + w.part);
    int32_t* pcount = reinterpret_cast<int32_t*>(base + w.pcount);
    double* pinertia = reinterpret_cast<double*>(base + w.pinertia);
    int32_t* pchanged = reinterpret_cast<int32_t*>(base + w.pchanged);
    double* shiftc = reinterpret_cast<double*>(base + w.shiftc);
    hipStream_t st = (hipStream_t)stream;
    MMVAE_LAUNCH(clust_centroids_kernel, dim3((unsigned)(CP / 16)), dim3(THREADS), 0, st, C, D, DP, centroids, cp, cnorm);
    MMVAE_LAUNCH_CHECK();
    int rc;
    switch (DP) {
        case 64: rc = launch_assign<64>(g, N, D, x, ldx, C, cp, cnorm, label, dist2, part, pcount, pinertia, pchanged, st); break;
        case 128: rc = launch_assign<128>(g, N, D, x, ldx, C, cp, cnorm, label, dist2, part, pcount, pinertia, pchanged, st); break;
        case 256: rc = launch_assign<256>(g, N, D, x, ldx, C, cp, cnorm, label, dist2, part, pcount, pinertia, pchanged, st); break;
        default: rc = launch_assign<512>(g, N, D, x, ldx, C, cp, cnorm, label, dist2, part, pcount, pinertia, pchanged, st); break;
    }
    if (rc != MMVAE_OK) return rc;
    MMVAE_LAUNCH(clust_means_kernel, dim3((unsigned)C), dim3(THREADS), 0, st, D, C, g.groups, centroids, part, pcount,
                 new_centroids, counts, shiftc);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(clust_stats_kernel, dim3(1), dim3(64), 0, st, C, g.groups, pinertia, pchanged, shiftc, counts,
                 static_cast<Stats*>(stats));
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_clust_seed_update_f32(int N, int D, const float* x, int64_t ldx, int row, int first, float* mind2,
                                           mmvae_stream_t stream) {
    if (N < 1 || D < 1 || D > MMVAE_CLUST_MAX_D || ldx < D || row < 0 || row >= N) return MMVAE_ERR_ARG;
    if (!x || !mind2) return MMVAE_ERR_ARG;
    const unsigned blocks = (unsigned)(((int64_t)N + 64 * WAVES - 1) / (64 * WAVES));
    MMVAE_LAUNCH(clust_seed_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, N, D, x, ldx, row, first, mind2);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
