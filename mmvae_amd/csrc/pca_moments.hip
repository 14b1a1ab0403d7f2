// The N-scale moments of PCA and principal-component regression (include/mmvae_pca.h) -> libmmvae_pca.so.
//
// Three entries: the per-class fp64 column sums of the centred rows (a sorted, segmented walk), the centred scatter
// matrix (a TN Gram on v_mfma_f32_16x16x4_f32: the ROWS of x are the K dimension, so a staged row is contiguous across
// the lanes), and the projection on the components (the same MFMA with the columns as K).  The exact-fp32 discipline is
// that of umap_knn.hip, sil_rows.hip and kmeans.hip: an MFMA accumulator element is one k-ordered fmaf chain, fp32 chains
// are short and join fp64 accumulators in a fixed order, and nothing is added atomically.
#include "common.h"
#include "../../include/mmvae_pca.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TS = 64;                     // side of an output tile of the scatter
constexpr int KR = 32;                     // rows of x per staged chunk
constexpr int LDT = TS + 16;               // floats per staged row: the rows k and k + 1 of an operand read sit 16 banks apart
constexpr int CHAIN = MMVAE_PCA_CHAIN;
constexpr int SEG = MMVAE_PCA_SEGMENT;
constexpr size_t TILE_BYTES = (size_t)TS * TS * sizeof(double);
static_assert(CHAIN % KR == 0 && CHAIN <= 1024, "a chain is a whole number of staged chunks");
static_assert(MMVAE_PCA_PARTIAL_CAP / TILE_BYTES >= 36, "one row range of the widest shape fits the cap");

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// ------------------------------------------------------------------------------------------------ 1. class sums
bool sums_shape_ok(int N, int D) { return N >= 1 && D >= 1 && D <= MMVAE_PCA_MAX_D; }
inline int n_segments(int N) { return (int)(((int64_t)N + SEG - 1) / SEG); }

// Wave threadIdx.y of workgroup blockIdx.x owns segment 4 blockIdx.x + threadIdx.y, its lane l the column
// 64 blockIdx.y + l: a load of one row is one 256-byte line.  The thread walks the segment's positions in ascending order
// (eight loads in flight at a time; the additions stay in order) and closes a piece wherever a run ends.  A run that lies
// inside the segment is written to sums_out; of the others at most one ENTERS the segment (piece 0) and at most one
// LEAVES it (piece 1; a run that does both is piece 0).
__global__ __launch_bounds__(THREADS) void pca_group_sums_kernel(int D, const float* __restrict__ x, int64_t ldx,
                                                                 const float* __restrict__ mean, int C,
                                                                 const int32_t* __restrict__ order,
                                                                 const int32_t* __restrict__ run_ptr,
                                                                 double* __restrict__ sums, double* __restrict__ part,
                                                                 int nseg) {
    const int seg = blockIdx.x * WAVES + threadIdx.y;
    const int d = blockIdx.y * 64 + threadIdx.x;
    if (seg >= nseg || d >= D) return;
    const int total = run_ptr[C];
    const int64_t k0 = (int64_t)seg * SEG;
    if (k0 >= total) return;
    const int64_t k1 = min((int64_t)total, k0 + SEG);
    // the run of position k0: run_ptr[lo] <= k0 < run_ptr[hi] throughout
    int lo = 0, hi = C;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (run_ptr[mid] <= k0) lo = mid;
        else hi = mid;
    }
    int c = lo;
    const float m = mean ? mean[d] : 0.f;
    const float* __restrict__ xd = x + d;
    int64_t k = k0;
    while (k < k1) {
        const int64_t s = run_ptr[c], e = run_ptr[c + 1];  // s <= k < e
        const int64_t stop = e < k1 ? e : k1;
        double acc = 0.0;
        for (; k + 8 <= stop; k += 8) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = xd[(int64_t)order[k + j] * ldx];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += (double)(t[j] - m);
        }
        for (; k < stop; ++k) acc += (double)(xd[(int64_t)order[k] * ldx] - m);
        if (s >= k0 && e <= k0 + SEG) sums[(int64_t)c * D + d] = acc;
        else part[((int64_t)seg * 2 + (s < k0 ? 0 : 1)) * D + d] = acc;
        if (k < k1) {  // the next run that is not empty
            ++c;
            while (c + 1 < C && run_ptr[c + 1] <= k) ++c;
        }
    }
}

// One thread per (class, column): zeros for an empty run, and for a run over several segments its pieces in ascending
// order.  (A run inside one segment was written by the walk.)
__global__ __launch_bounds__(THREADS) void pca_group_finish_kernel(int D, int C, const int32_t* __restrict__ run_ptr,
                                                                   const double* __restrict__ part, double* __restrict__ sums) {
    const int64_t at = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (at >= (int64_t)C * D) return;
    const int c = (int)(at / D), d = (int)(at - (int64_t)c * D);
    const int s = run_ptr[c], e = run_ptr[c + 1];
    if (s >= e) {
        sums[at] = 0.0;
        return;
    }
    const int b_lo = s / SEG, b_hi = (e - 1) / SEG;
    if (b_lo == b_hi) return;
    double acc = 0.0;
    acc += part[((int64_t)b_lo * 2 + 1) * D + d];
    for (int b = b_lo + 1; b <= b_hi; ++b) acc += part[((int64_t)b * 2) * D + d];
    sums[at] = acc;
}

// ------------------------------------------------------------------------------------------------ 2. scatter
bool scatter_shape_ok(int N, int D, int M) {
    return N >= 1 && D >= 1 && M >= 0 && M <= MMVAE_PCA_MAX_COV && D <= MMVAE_PCA_MAX_D && D + M <= MMVAE_PCA_MAX_D;
}

// The grid, a function of (N, W) alone: the tiles on and above the diagonal times the row ranges.  A range is a whole
// number of chains, two at least where there are two, and more while the fp64 tiles of all workgroups exceed the cap.
struct ScatterGrid {
    int nt, tiles, chains, per, ranges;
};
ScatterGrid scatter_grid(int N, int W) {
    ScatterGrid g;
    g.nt = (W + TS - 1) / TS;
    g.tiles = g.nt * (g.nt + 1) / 2;
    g.chains = (int)(((int64_t)N + CHAIN - 1) / CHAIN);
    const int cap = (int)(MMVAE_PCA_PARTIAL_CAP / (TILE_BYTES * (size_t)g.tiles));
    int want = (g.chains + 1) / 2;
    if (want > cap) want = cap;
    g.per = (g.chains + want - 1) / want;
    g.ranges = (g.chains + g.per - 1) / g.per;
    return g;
}

// tile t of the upper triangle, row after row: (0,0) (0,1) .. (0,nt-1) (1,1) ..
__device__ __forceinline__ void tile_of(int t, int nt, int& tu, int& tv) {
    tu = 0;
    while (t >= nt - tu) {
        t -= nt - tu;
        ++tu;
    }
    tv = tu + t;
}

// Column w of the augmented row: where it starts, its row stride, and whether it exists.
struct Column {
    const float* p;
    int64_t ld;
    float mean;
    bool live;
};
__device__ __forceinline__ Column column_of(int w, int D, int W, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                            const float* mean) {
    Column c;
    c.live = w < W;
    c.p = w < D ? x + w : y + (w - D);
    c.ld = w < D ? ldx : ldy;
    c.mean = c.live ? mean[w] : 0.f;
    if (!c.live) c.p = x, c.ld = 0;
    return c;
}

// Workgroup (t, g) computes output tile t over the chains [g per, min(chains, (g + 1) per)).  Per chunk of KR rows every
// thread centres column (threadIdx & 63) of both panels for the rows (threadIdx >> 6) + 4 j and stages them as [row][column]
// (rows past the chain's end and columns past W are exact zeros: fmaf(0, 0, acc) = acc); the next chunk's loads are in
// flight while this one is multiplied.  Wave w holds the tile's rows 16 w .. + 15: the A operand of lane l is column
// 16 w + (l & 15) of the u panel at row 4 kk + (l >> 4), the B operands the columns 16 n + (l & 15) of the v panel, and
// accumulator element e of block n is S(u = 16 w + 4 (l >> 4) + e, v = 16 n + (l & 15)).  A diagonal tile stages one panel.
__global__ __launch_bounds__(THREADS) void pca_scatter_kernel(int N, int D, int W, const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ y, int64_t ldy,
                                                              const float* __restrict__ mean, double* __restrict__ part,
                                                              int nt, int chains, int per) {
    __shared__ float As[KR * LDT], Bs[KR * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane & 15, q = lane >> 4;
    int tu, tv;
    tile_of(blockIdx.x, nt, tu, tv);
    const bool diag = tu == tv;
    const int col = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const Column ca = column_of(tu * TS + col, D, W, x, ldx, y, ldy, mean);
    const Column cb = column_of(tv * TS + col, D, W, x, ldx, y, ldy, mean);
    const float* __restrict__ Bsel = diag ? As : Bs;

    double accd[4][4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) accd[n][e] = 0.0;

    const int c_begin = blockIdx.y * per, c_end = min(chains, c_begin + per);
    for (int ch = c_begin; ch < c_end; ++ch) {
        const int64_t row0 = (int64_t)ch * CHAIN;
        const int64_t row_end = min((int64_t)N, row0 + CHAIN);
        const int nchunks = (int)((row_end - row0 + KR - 1) / KR);
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        float ra[KR / WAVES], rb[KR / WAVES];
        auto load = [&](int chunk) {
#pragma unroll
            for (int j = 0; j < KR / WAVES; ++j) {
                const int64_t r = row0 + (int64_t)chunk * KR + r0 + WAVES * j;
                const bool in = r < row_end;
                ra[j] = (in && ca.live) ? ca.p[r * ca.ld] - ca.mean : 0.f;
                rb[j] = (in && cb.live && !diag) ? cb.p[r * cb.ld] - cb.mean : 0.f;
            }
        };
        load(0);
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            __syncthreads();  // (the chunk before this one has been multiplied)
#pragma unroll
            for (int j = 0; j < KR / WAVES; ++j) {
                As[(r0 + WAVES * j) * LDT + col] = ra[j];
                if (!diag) Bs[(r0 + WAVES * j) * LDT + col] = rb[j];
            }
            __syncthreads();
            if (chunk + 1 < nchunks) load(chunk + 1);
            const float* __restrict__ A = As + q * LDT + 16 * wave + cl;
            const float* __restrict__ B = Bsel + q * LDT + cl;
#pragma unroll
            for (int kk = 0; kk < KR / 4; ++kk) {
                const float a = A[4 * kk * LDT];
                float b[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) b[n] = B[4 * kk * LDT + 16 * n];
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[n], acc[n], 0, 0, 0);
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) accd[n][e] += (double)acc[n][e];
    }
    double* __restrict__ mine = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (TS * TS);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) mine[(16 * wave + 4 * q + e) * TS + 16 * n + cl] = accd[n][e];
}

// Workgroup (t, j) adds, for 256 elements of tile t, the ranges' partials from zero in ascending order, and writes the
// element and its mirror image.  Of a diagonal tile the elements u <= v are kept.
__global__ __launch_bounds__(THREADS) void pca_scatter_finish_kernel(int W, int nt, int ranges, const double* __restrict__ part,
                                                                     double* __restrict__ out) {
    int tu, tv;
    tile_of(blockIdx.x, nt, tu, tv);
    const int at = blockIdx.y * THREADS + threadIdx.x;
    const int u = tu * TS + (at >> 6), v = tv * TS + (at & 63);
    if (u >= W || v >= W || (tu == tv && u > v)) return;
    const double* __restrict__ p = part + (int64_t)blockIdx.x * (TS * TS) + at;
    const int64_t step = (int64_t)gridDim.x * (TS * TS);
    double s = 0.0;
    int g = 0;
    for (; g + 8 <= ranges; g += 8) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = p[(g + j) * step];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += t[j];
    }
    for (; g < ranges; ++g) s += p[g * step];
    out[(int64_t)u * W + v] = s;
    out[(int64_t)v * W + u] = s;
}

// ------------------------------------------------------------------------------------------------ 3. projection
// A workgroup owns 64 rows.  Per chunk of 64 columns every thread centres column (threadIdx & 63) of the rows
// (threadIdx >> 6) + 4 j as it loads them -- whole 256-byte lines, whatever ldx is -- and stages them [row][column]; the
// components of the tile are staged the same way ([component][column]).  66 floats per staged row: the 16 rows of an
// operand read sit 2 banks apart, beside the two columns of a half wave.  Wave w then holds the rows 16 w .. + 15 as A
// operands (lane l: row l & 15, column 4 kk + (l >> 4)) and the components 16 n + (l & 15) as B operands.  Rows past N,
// columns past D and components past P are exact zeros: fmaf(0, 0, acc) = acc, so a score is the chain over its D
// columns.  NB = 16-component blocks of a tile; a wider P walks tiles and stages the rows again (from the L2).
constexpr int LDP = 64 + 2;
template <int NB>
__global__ __launch_bounds__(THREADS) void pca_project_kernel(int N, int D, const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ mean, int P,
                                                              const float* __restrict__ comp, float* __restrict__ scores,
                                                              int64_t lds) {
    __shared__ float Xs[64 * LDP], Bs[16 * NB * LDP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane & 15, q = lane >> 4;
    const int col = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    for (int p0 = 0; p0 < P; p0 += 16 * NB) {
        f32x4 acc[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += 64) {
            const int k = k0 + col;
            const bool in = k < D;
            const float m = in ? mean[k] : 0.f;
            float xr[16], br[4 * NB];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int64_t row = row0 + r0 + WAVES * j;
                xr[j] = (in && row < N) ? x[row * ldx + k] - m : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4 * NB; ++j) {
                const int p = p0 + r0 + WAVES * j;
                br[j] = (in && p < P) ? comp[(int64_t)p * D + k] : 0.f;
            }
            __syncthreads();  // (the chunk before this one has been multiplied)
#pragma unroll
            for (int j = 0; j < 16; ++j) Xs[(r0 + WAVES * j) * LDP + col] = xr[j];
#pragma unroll
            for (int j = 0; j < 4 * NB; ++j) Bs[(r0 + WAVES * j) * LDP + col] = br[j];
            __syncthreads();
            const float* __restrict__ A = Xs + (16 * wave + cl) * LDP + q;
            const float* __restrict__ B = Bs + cl * LDP + q;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float a = A[4 * kk];
                float b[NB];
#pragma unroll
                for (int n = 0; n < NB; ++n) b[n] = B[16 * n * LDP + 4 * kk];
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[n], acc[n], 0, 0, 0);
            }
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int p = p0 + 16 * n + cl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t row = row0 + 16 * wave + 4 * q + e;
                if (row < N && p < P) scores[row * lds + p] = acc[n][e];
            }
        }
    }
}

template <int NB>
int launch_project(int N, int D, const float* x, int64_t ldx, const float* mean, int P, const float* comp, float* scores,
                   int64_t lds, hipStream_t st) {
    const unsigned blocks = (unsigned)(((int64_t)N + 63) / 64);
    MMVAE_LAUNCH((pca_project_kernel<NB>), dim3(blocks), dim3(THREADS), 0, st, N, D, x, ldx, mean, P, comp, scores, lds);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

}  // namespace

extern "C" int mmvae_pca_abi_version(void) { return MMVAE_PCA_ABI_VERSION; }
extern "C" const char* mmvae_pca_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_pca_group_sums_workspace_bytes(int N, int D) {
    if (!sums_shape_ok(N, D)) return 0;
    return up16((size_t)n_segments(N) * 2 * (size_t)D * sizeof(double));
}

extern "C" int mmvae_pca_group_sums_f64(int N, int D, const float* x, int64_t ldx, const float* mean, int C,
                                        const int32_t* order, const int32_t* run_ptr, double* sums_out, void* workspace,
                                        size_t workspace_bytes, mmvae_stream_t stream) {
    if (!sums_shape_ok(N, D) || ldx < D || C < 1 || C > N) return MMVAE_ERR_ARG;
    if ((int64_t)C * D > MMVAE_PCA_MAX_SUMS) return MMVAE_ERR_ARG;  // (the finishing launch has a thread per element)
    if (!x || !order || !run_ptr || !sums_out || !workspace) return MMVAE_ERR_ARG;
    if (workspace_bytes < mmvae_pca_group_sums_workspace_bytes(N, D) || !aligned16(workspace)) return MMVAE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nseg = n_segments(N);
    double* part = static_cast<double*>(workspace);
    MMVAE_LAUNCH(pca_group_sums_kernel, dim3((unsigned)((nseg + WAVES - 1) / WAVES), (unsigned)((D + 63) / 64)),
                 dim3(64, WAVES), 0, st, D, x, ldx, mean, C, order, run_ptr, sums_out, part, nseg);
    MMVAE_LAUNCH_CHECK();
    const unsigned blocks = (unsigned)(((int64_t)C * D + THREADS - 1) / THREADS);
    MMVAE_LAUNCH(pca_group_finish_kernel, dim3(blocks), dim3(THREADS), 0, st, D, C, run_ptr, part, sums_out);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" size_t mmvae_pca_scatter_workspace_bytes(int N, int D, int M) {
    if (!scatter_shape_ok(N, D, M)) return 0;
    const ScatterGrid g = scatter_grid(N, D + M);
    return up16((size_t)g.tiles * g.ranges * TILE_BYTES);
}

extern "C" int mmvae_pca_scatter_f32(int N, int D, const float* x, int64_t ldx, int M, const float* y, int64_t ldy,
                                     const float* mean, double* scatter_out, void* workspace, size_t workspace_bytes,
                                     mmvae_stream_t stream) {
    if (!scatter_shape_ok(N, D, M) || ldx < D) return MMVAE_ERR_ARG;
    if (M > 0 && (!y || ldy < M)) return MMVAE_ERR_ARG;
    if (!x || !mean || !scatter_out || !workspace) return MMVAE_ERR_ARG;
    if (workspace_bytes < mmvae_pca_scatter_workspace_bytes(N, D, M) || !aligned16(workspace)) return MMVAE_ERR_ARG;
    const int W = D + M;
    const ScatterGrid g = scatter_grid(N, W);
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(workspace);
    MMVAE_LAUNCH(pca_scatter_kernel, dim3((unsigned)g.tiles, (unsigned)g.ranges), dim3(THREADS), 0, st, N, D, W, x, ldx,
                 M > 0 ? y : x, M > 0 ? ldy : 0, mean, part, g.nt, g.chains, g.per);
    MMVAE_LAUNCH_CHECK();
    MMVAE_LAUNCH(pca_scatter_finish_kernel, dim3((unsigned)g.tiles, (unsigned)(TS * TS / THREADS)), dim3(THREADS), 0, st, W,
                 g.nt, g.ranges, part, scatter_out);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

extern "C" int mmvae_pca_project_f32(int N, int D, const float* x, int64_t ldx, const float* mean, int P,
                                     const float* components, float* scores, int64_t lds, mmvae_stream_t stream) {
    if (N < 1 || D < 1 || D > MMVAE_PCA_MAX_D || ldx < D || P < 1 || P > D || lds < P) return MMVAE_ERR_ARG;
    if (!x || !mean || !components || !scores) return MMVAE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (P + 15) / 16;
    switch (nb < 4 ? nb : 4) {
        case 1: return launch_project<1>(N, D, x, ldx, mean, P, components, scores, lds, st);
        case 2: return launch_project<2>(N, D, x, ldx, mean, P, components, scores, lds, st);
        case 3: return launch_project<3>(N, D, x, ldx, mean, P, components, scores, lds, st);
        default: return launch_project<4>(N, D, x, ldx, mean, P, components, scores, lds, st);
    }
}
