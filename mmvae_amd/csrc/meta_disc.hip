// libmmvae_disc.so (include/mmvae_disc.h): a meta-discriminator behind its first layer -- forward, loss and backward.
#include "common.h"
#include "../../include/mmvae_disc.h"

namespace {

constexpr int ROWS = MMVAE_DISC_TILE_ROWS;  // rows per tile
constexpr int THREADS = 256;
constexpr int TLD = 20;  // row length of the [column][ROWS] images: 16-byte rows of 4 for ds_read_b128, 80-byte pitch
static_assert(ROWS == 16, "the row groups below are four groups of four rows");

struct Tail {
    int B, H1, H2, ntiles, train;
    const float *pre1, *W2, *b2, *W3, *b3, *y;
    float *p, *dpre1, *ws;
    int64_t ld1, ldd;
};

// Floats of one tile's record in the workspace: dW2 [H2*H1] | db2 [H2] | dW3 [H2] | db1 [H1] | db3, loss, hits.
__host__ __device__ inline int64_t record_floats(int H1, int H2) { return ((int64_t)H1 * H2 + 2 * H2 + H1 + 3 + 3) / 4 * 4; }

// sigmoid(x), sigmoid(-x) and their product, none of them through a cancelling 1 - sigmoid.
__device__ __forceinline__ void sigmoid3(float x, float& s, float& sneg, float& prod) {
    const float e = expf(-fabsf(x));
    const float big = 1.f / (1.f + e), small = e * big;
    s = x >= 0.f ? big : small;
    sneg = x >= 0.f ? small : big;
    prod = big * small;
}
__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// LDS carve (floats).  w2s [H2][ldw] (ldw odd: a column of W2 across the lanes is conflict-free) | h1s [ROWS][H1] |
// g1s [ROWS][H1] | h1t [H1][TLD] (after the forward: dps [ROWS][H1]) | h2s [ROWS][H2] | dat [H2][TLD] | b2s | w3s | row words
struct Carve {
    int ldw, w2s, h1s, g1s, h1t, h2s, dat, b2s, w3s, rowv, total;
};
__host__ __device__ inline Carve carve(int H1, int H2) {
    Carve c;
    c.ldw = H1 | 1;
    int o = 0;
    auto take = [&o](int n) { int at = o; o += (n + 3) / 4 * 4; return at; };
    c.h1t = take(H1 * TLD);  // (first: 16-byte aligned rows)
    c.dat = take(H2 * TLD);
    c.w2s = take(H2 * c.ldw);
    c.h1s = take(ROWS * H1);
    c.g1s = take(ROWS * H1);
    c.h2s = take(ROWS * H2);
    c.b2s = take(H2);
    c.w3s = take(H2);
    c.rowv = take(3 * ROWS);  // ds, loss, hit per row
    c.total = o;
    return c;
}

__global__ __launch_bounds__(THREADS) void disc_tail_kernel(Tail a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H1 = a.H1, H2 = a.H2, t = threadIdx.x;
    const Carve c = carve(H1, H2);
    float* w2s = lds + c.w2s;
    float* h1s = lds + c.h1s;
    float* g1s = lds + c.g1s;
    float* h1t = lds + c.h1t;
    float* dps = h1t;  // the forward's transposed image is dead once h2 exists
    float* h2s = lds + c.h2s;
    float* dat = lds + c.dat;
    float* b2s = lds + c.b2s;
    float* w3s = lds + c.w3s;
    float* dss = lds + c.rowv;
    float* rloss = dss + ROWS;
    float* rhit = rloss + ROWS;
    const int ldw = c.ldw;
    const int64_t S = record_floats(H1, H2);
    const int64_t o_db2 = (int64_t)H1 * H2, o_dw3 = o_db2 + H2, o_db1 = o_dw3 + H2, o_db3 = o_db1 + H1;

    for (int i = t; i < H1 * H2; i += THREADS) w2s[(i / H1) * ldw + i % H1] = a.W2[i];
    for (int j = t; j < H2; j += THREADS) {
        b2s[j] = a.b2[j];
        w3s[j] = a.W3[j];
    }
    const float b3 = a.b3[0];
    const float Bf = (float)a.B;

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (int64_t)tile * ROWS;
        float* rec = a.ws + (int64_t)tile * S;
        __syncthreads();  // the weights are in; the previous tile's readers are done
        // ---- h1 = sigmoid(pre1) and h1 (1 - h1), rows past B as zeros
        for (int i = t; i < ROWS * H1; i += THREADS) {
            const int r = i / H1, k = i % H1;
            float h = 0.f, hn, g = 0.f;
            if (row0 + r < a.B) sigmoid3(a.pre1[(row0 + r) * a.ld1 + k], h, hn, g);
            h1s[i] = h;
            g1s[i] = g;
            h1t[k * TLD + r] = h;
        }
        __syncthreads();
        // ---- h2 = sigmoid(h1 W2^T + b2): a unit is (column j, four rows), k in order
        for (int u = t; u < 4 * H2; u += THREADS) {
            const int j = u % H2, rg = u / H2;
            const float* w = w2s + j * ldw;
            const float bj = b2s[j];
            float acc0 = bj, acc1 = bj, acc2 = bj, acc3 = bj;
#pragma unroll 4
            for (int k = 0; k < H1; ++k) {
                const float wk = w[k];
                const f32x4 h = *reinterpret_cast<const f32x4*>(h1t + k * TLD + rg * 4);
                acc0 = fmaf(wk, h.x, acc0);
                acc1 = fmaf(wk, h.y, acc1);
                acc2 = fmaf(wk, h.z, acc2);
                acc3 = fmaf(wk, h.w, acc3);
            }
            const float acc[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float h, hn, g;
                sigmoid3(acc[q], h, hn, g);
                h2s[(rg * 4 + q) * H2 + j] = h;
                dat[j * TLD + rg * 4 + q] = g;  // h2 (1 - h2) for now
            }
        }
        __syncthreads();
        // ---- s = h2 . W3 + b3, p, the row's loss and ds: wave w takes rows 4w .. 4w + 3
        {
            const int wave = t >> 6, lane = t & 63;
            for (int q = 0; q < 4; ++q) {
                const int r = wave * 4 + q;
                float part = 0.f;
                for (int j = lane; j < H2; j += 64) part = fmaf(h2s[r * H2 + j], w3s[j], part);
                const float s = wave_sum(part) + b3;
                if (lane == 0) {
                    float ds = 0.f, loss = 0.f, hit = 0.f;
                    if (row0 + r < a.B) {
                        float p, pn, g;
                        sigmoid3(s, p, pn, g);
                        if (a.p) a.p[row0 + r] = p;
                        if (a.y) {
                            const float y = a.y[row0 + r];
                            loss = y * fminf(softplus(-s), 100.f) + (1.f - y) * fminf(softplus(s), 100.f);
                            hit = ((p > 0.5f) == (y > 0.5f)) ? 1.f : 0.f;
                            ds = ((1.f - y) * p - y * pn) / Bf;
                        }
                    }
                    dss[r] = ds;
                    rloss[r] = loss;
                    rhit[r] = hit;
                }
            }
        }
        __syncthreads();
        if (t == THREADS - 1) {  // the tile's loss, hit count and db3, rows in order
            float l = 0.f, h = 0.f, d = 0.f;
            for (int r = 0; r < ROWS; ++r) {
                l += rloss[r];
                h += rhit[r];
                d += dss[r];
            }
            rec[o_db3] = d;
            rec[o_db3 + 1] = l;
            rec[o_db3 + 2] = h;
        }
        if (!a.train) continue;
        // ---- dW3 partial (reads h2), then da2 = ds W3 h2 (1 - h2) in place of h2 (1 - h2)
        for (int j = t; j < H2; j += THREADS) {
            float d = 0.f;
            for (int r = 0; r < ROWS; ++r) d = fmaf(dss[r], h2s[r * H2 + j], d);
            rec[o_dw3 + j] = d;
        }
        for (int i = t; i < ROWS * H2; i += THREADS) {
            const int j = i / ROWS, r = i % ROWS;
            dat[j * TLD + r] = dss[r] * w3s[j] * dat[j * TLD + r];
        }
        __syncthreads();
        // ---- db2 partial
        for (int j = t; j < H2; j += THREADS) {
            float d = 0.f;
            for (int r = 0; r < ROWS; ++r) d += dat[j * TLD + r];
            rec[o_db2 + j] = d;
        }
        // ---- dW2 partial [H2][H1]: a unit keeps column k of h1 in registers and walks every JG-th j
        {
            const int JG = (THREADS + H1 - 1) / H1;
            for (int u = t; u < H1 * JG; u += THREADS) {
                const int k = u % H1, jg = u / H1;
                float h[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) h[r] = h1s[r * H1 + k];
                for (int j = jg; j < H2; j += JG) {
                    const f32x4* d4 = reinterpret_cast<const f32x4*>(dat + j * TLD);
                    float acc = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 d = d4[q];
                        acc = fmaf(d.x, h[4 * q + 0], acc);
                        acc = fmaf(d.y, h[4 * q + 1], acc);
                        acc = fmaf(d.z, h[4 * q + 2], acc);
                        acc = fmaf(d.w, h[4 * q + 3], acc);
                    }
                    rec[(int64_t)j * H1 + k] = acc;
                }
            }
        }
        // ---- dpre1 = (da2 W2) h1 (1 - h1): a unit is (column k, four rows), j in order
        for (int u = t; u < 4 * H1; u += THREADS) {
            const int k = u % H1, rg = u / H1;
            float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll 4
            for (int j = 0; j < H2; ++j) {
                const float wj = w2s[j * ldw + k];
                const f32x4 d = *reinterpret_cast<const f32x4*>(dat + j * TLD + rg * 4);
                acc0 = fmaf(wj, d.x, acc0);
                acc1 = fmaf(wj, d.y, acc1);
                acc2 = fmaf(wj, d.z, acc2);
                acc3 = fmaf(wj, d.w, acc3);
            }
            const float acc[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = rg * 4 + q;
                const float dp = acc[q] * g1s[r * H1 + k];
                dps[r * H1 + k] = dp;
                if (row0 + r < a.B) a.dpre1[(row0 + r) * a.ldd + k] = dp;
            }
        }
        __syncthreads();
        // ---- db1 partial
        for (int k = t; k < H1; k += THREADS) {
            float d = 0.f;
            for (int r = 0; r < ROWS; ++r) d += dps[r * H1 + k];
            rec[o_db1 + k] = d;
        }
    }
}

// Adds the tiles' records in tile order; thread = one word of the record.
__global__ __launch_bounds__(THREADS) void disc_sum_kernel(int B, int H1, int H2, int ntiles, int train,
                                                           const float* __restrict__ ws, float* __restrict__ out,
                                                           float* __restrict__ db1, float* __restrict__ dW2,
                                                           float* __restrict__ db2, float* __restrict__ dW3,
                                                           float* __restrict__ db3) {
    const int64_t S = record_floats(H1, H2);
    const int64_t o_db2 = (int64_t)H1 * H2, o_dw3 = o_db2 + H2, o_db1 = o_dw3 + H2, o_db3 = o_db1 + H1;
    int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (!train) e += o_db3 + 1;  // loss and hits only
    if (e >= o_db3 + 3) return;
    float acc = 0.f;
    for (int tile = 0; tile < ntiles; ++tile) acc += ws[(int64_t)tile * S + e];
    if (e < o_db2)
        dW2[e] = acc;
    else if (e < o_dw3)
        db2[e - o_db2] = acc;
    else if (e < o_db1)
        dW3[e - o_dw3] = acc;
    else if (e < o_db3)
        db1[e - o_db1] = acc;
    else if (e == o_db3)
        db3[0] = acc;
    else if (out)
        out[e - o_db3 - 1] = acc / (float)B;
}

bool shape_ok(int B, int H1, int H2) {
    return B >= 1 && H1 >= 1 && H1 <= MMVAE_DISC_MAX_H1 && H2 >= 1 && H2 <= MMVAE_DISC_MAX_H2 &&
           (int64_t)H1 * H2 <= MMVAE_DISC_MAX_W2;
}

}  // namespace

extern "C" int mmvae_disc_abi_version(void) { return MMVAE_DISC_ABI_VERSION; }
extern "C" const char* mmvae_disc_build_arch(void) { return "gfx950"; }

extern "C" size_t mmvae_disc_tail_workspace_bytes(int B, int H1, int H2) {
    if (!shape_ok(B, H1, H2)) return 0;
    const int64_t ntiles = ((int64_t)B + ROWS - 1) / ROWS;
    return (size_t)(ntiles * record_floats(H1, H2)) * sizeof(float);
}

extern "C" int mmvae_disc_tail_f32(int B, int H1, int H2, const float* pre1, int64_t ld1, const float* W2, const float* b2,
                                   const float* W3, const float* b3, const float* y, float* p, float* out, float* dpre1,
                                   int64_t ldd, float* db1, float* dW2, float* db2, float* dW3, float* db3, void* workspace,
                                   size_t workspace_bytes, mmvae_stream_t stream) {
    if (!shape_ok(B, H1, H2)) return MMVAE_ERR_ARG;
    if (!pre1 || ld1 < H1 || !W2 || !b2 || !W3 || !b3) return MMVAE_ERR_ARG;
    const bool train = dpre1 != nullptr;
    if (train) {
        if (ldd < H1 || !db1 || !dW2 || !db2 || !dW3 || !db3 || !y || !out) return MMVAE_ERR_ARG;
    } else {
        if (db1 || dW2 || db2 || dW3 || db3) return MMVAE_ERR_ARG;
        if (!y && (out || !p)) return MMVAE_ERR_ARG;
        if (!p && !out) return MMVAE_ERR_ARG;
    }
    const size_t need = mmvae_disc_tail_workspace_bytes(B, H1, H2);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return MMVAE_ERR_ARG;

    static bool attr = false;  // (a property of the code object, not of a call: dynamic LDS past 64 KiB)
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(disc_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 2048) != hipSuccess)
            return MMVAE_ERR_LAUNCH;
        attr = true;
    }
    Tail a;
    a.B = B;
    a.H1 = H1;
    a.H2 = H2;
    a.ntiles = (int)(((int64_t)B + ROWS - 1) / ROWS);
    a.train = train ? 1 : 0;
    a.pre1 = pre1;
    a.W2 = W2;
    a.b2 = b2;
    a.W3 = W3;
    a.b3 = b3;
    a.y = y;
    a.p = p;
    a.dpre1 = dpre1;
    a.ws = static_cast<float*>(workspace);
    a.ld1 = ld1;
    a.ldd = ldd;
    const Carve c = carve(H1, H2);
    hipStream_t st = (hipStream_t)stream;
    const int grid = a.ntiles < MMVAE_DISC_GRID_CAP ? a.ntiles : MMVAE_DISC_GRID_CAP;
    MMVAE_LAUNCH(disc_tail_kernel, dim3(grid), dim3(THREADS), (size_t)c.total * sizeof(float), st, a);
    MMVAE_LAUNCH_CHECK();
    if (train || out) {
        const int64_t words = train ? record_floats(H1, H2) : 2;
        MMVAE_LAUNCH(disc_sum_kernel, dim3((unsigned)((words + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, B, H1, H2,
                     a.ntiles, a.train, (const float*)a.ws, out, db1, dW2, db2, dW3, db3);
        MMVAE_LAUNCH_CHECK();
    }
    return MMVAE_OK;
}
