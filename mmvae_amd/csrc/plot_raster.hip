// Category scatter plots: per-pixel, per-class point counts and their composite (include/mmvae_plot.h) -> libmmvae_plot.so.
#include "common.h"
#include "../../include/mmvae_plot.h"

// The pixel mapping is stated operation by operation: no multiply and add of it may be fused.
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_GROUPS = 2048;  // workgroups of the count pass: 8 per CU, each strides over the points
constexpr uint32_t NO_KEY = 0xffffffffu;
// What MMVAE_PLOT_COUNT_DEFAULT means: decided by the A/B of tools/bench_umap_plot.py (profiles/umap_plot.txt).
constexpr bool DEFAULT_AGG = false;

struct View {
    float a00, a01, a02, b0, a10, a11, a12, b1;
};

struct Raster {
    int n_classes, W, H, m, lo, hi;  // the block: cx - lo .. cx + hi
};

// A product and a sum of their own: written out here, under the pragma, so that nothing fuses them.
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

__device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// (class, centre pixel) of one point as a 32-bit key, NO_KEY for a dropped point.  cx + 8 and cy + 8 lie in
// 0 .. MMVAE_PLOT_MAX_SIDE + 11 < 2^14 and the class in 0 .. 15, so no kept point has the key NO_KEY.
template <int DIMS>
__device__ __forceinline__ uint32_t key_of(float x, float y, float z, int code, const View& vw, const Raster& r) {
    bool ok = (uint32_t)code < (uint32_t)r.n_classes && finite(x) && finite(y);
    float u = add_rn(mul_rn(vw.a00, x), mul_rn(vw.a01, y));
    float v = add_rn(mul_rn(vw.a10, x), mul_rn(vw.a11, y));
    if (DIMS == 3) {
        ok = ok && finite(z);
        u = add_rn(u, mul_rn(vw.a02, z));
        v = add_rn(v, mul_rn(vw.a12, z));
    }
    u = add_rn(u, vw.b0);
    v = add_rn(v, vw.b1);
    const float fu = floorf(u), fv = floorf(v);
    // comparisons between floats (NaN and +-inf fail them); the integer conversion below sees only values that passed
    ok = ok && finite(u) && finite(v) && fu >= -(float)r.hi && fu <= (float)(r.W - 1 + r.lo) && fv >= -(float)r.hi &&
         fv <= (float)(r.H - 1 + r.lo);
    if (!ok) return NO_KEY;
    const int cx = (int)fu, cy = (int)fv;
    return ((uint32_t)code << 28) | ((uint32_t)(cy + 8) << 14) | (uint32_t)(cx + 8);
}

// One point per lane, every lane of the wave in the call.  AGG: the lanes that share the first pending lane's key hand
// their number to that lane; that repeats while it pays (a round that took fewer than 8 lanes ends it, 4 rounds at most)
// and what is left adds 1 each.  Then every lane that still holds a number adds it to the pixels of its block.
template <bool AGG>
__device__ __forceinline__ void deposit(uint32_t key, const Raster& r, uint32_t* __restrict__ counts, int lane) {
    uint32_t add = 1u;
    bool mine = key != NO_KEY;
    if (AGG) {
        unsigned long long todo = __ballot(mine);
        mine = false;
        for (int round = 0; round < 4 && todo; ++round) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t lk = (uint32_t)__shfl((int)key, leader);
            const unsigned long long same = __ballot(key == lk) & todo;
            if (lane == leader) {
                mine = true;
                add = (uint32_t)__popcll(same);
            }
            todo &= ~same;
            if (__popcll(same) < 8) break;
        }
        if ((todo >> lane) & 1ull) mine = true;  // (add is still 1)
    }
    if (!mine) return;
    const int c = (int)(key >> 28), cy = (int)((key >> 14) & 0x3fffu) - 8, cx = (int)(key & 0x3fffu) - 8;
    const int x0 = max(cx - r.lo, 0), x1 = min(cx + r.hi, r.W - 1);
    const int y0 = max(cy - r.lo, 0), y1 = min(cy + r.hi, r.H - 1);
    uint32_t* plane = counts + (size_t)c * r.H * r.W;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) atomicAdd(&plane[(size_t)y * r.W + x], add);  // (result unused: no-return atomic)
}

// PACKED: ld == DIMS and both arrays 16-byte aligned -- a lane takes four points from 16-byte loads (two float4 for
// dims 2, three for dims 3, one int4 of codes); the last n % 4 points go element by element through the first wave of
// workgroup 0.  Otherwise one point per lane and pass, read element by element with the leading dimension.
template <int DIMS, bool PACKED, bool AGG>
__global__ __launch_bounds__(THREADS) void plot_count_kernel(int64_t n, const float* __restrict__ points, int64_t ld,
                                                             const int32_t* __restrict__ codes, View vw, Raster r,
                                                             uint32_t* __restrict__ counts) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    if (PACKED) {
        const int64_t n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(points);
        const int4* c4 = reinterpret_cast<const int4*>(codes);
        for (int64_t base = (int64_t)blockIdx.x * THREADS; base < n4; base += stride) {  // (uniform over the workgroup)
            const int64_t g = base + tid;
            uint32_t k0 = NO_KEY, k1 = NO_KEY, k2 = NO_KEY, k3 = NO_KEY;
            if (g < n4) {
                const int4 c = c4[g];
                if (DIMS == 2) {
                    const float4 a = p4[2 * g], b = p4[2 * g + 1];
                    k0 = key_of<2>(a.x, a.y, 0.f, c.x, vw, r);
                    k1 = key_of<2>(a.z, a.w, 0.f, c.y, vw, r);
                    k2 = key_of<2>(b.x, b.y, 0.f, c.z, vw, r);
                    k3 = key_of<2>(b.z, b.w, 0.f, c.w, vw, r);
                } else {
                    const float4 a = p4[3 * g], b = p4[3 * g + 1], d = p4[3 * g + 2];
                    k0 = key_of<3>(a.x, a.y, a.z, c.x, vw, r);
                    k1 = key_of<3>(a.w, b.x, b.y, c.y, vw, r);
                    k2 = key_of<3>(b.z, b.w, d.x, c.z, vw, r);
                    k3 = key_of<3>(d.y, d.z, d.w, c.w, vw, r);
                }
            }
            deposit<AGG>(k0, r, counts, lane);
            deposit<AGG>(k1, r, counts, lane);
            deposit<AGG>(k2, r, counts, lane);
            deposit<AGG>(k3, r, counts, lane);
        }
        if (blockIdx.x == 0 && tid < 64) {  // (the whole first wave: at most 3 points)
            const int64_t i = 4 * n4 + tid;
            uint32_t k = NO_KEY;
            if (i < n) {
                const float* p = points + (size_t)i * DIMS;
                k = key_of<DIMS>(p[0], p[1], DIMS == 3 ? p[2] : 0.f, codes[i], vw, r);
            }
            deposit<AGG>(k, r, counts, lane);
        }
    } else {
        for (int64_t base = (int64_t)blockIdx.x * THREADS; base < n; base += stride) {
            const int64_t i = base + tid;
            uint32_t k = NO_KEY;
            if (i < n) {
                const float* p = points + (size_t)i * (size_t)ld;
                k = key_of<DIMS>(p[0], p[1], DIMS == 3 ? p[2] : 0.f, codes[i], vw, r);
            }
            deposit<AGG>(k, r, counts, lane);
        }
    }
}

// One lane per pixel.  Plane c of the counts is read at the lane's pixel: consecutive lanes, consecutive words of a row.
__global__ __launch_bounds__(THREADS) void plot_composite_kernel(const uint32_t* __restrict__ counts, int n_classes,
                                                                 int64_t n_pix, const float* __restrict__ colors,
                                                                 float log2_keep, float bg_r, float bg_g, float bg_b,
                                                                 uchar4 bg_bytes, uchar4* __restrict__ rgba) {
    __shared__ float s_col[MMVAE_PLOT_MAX_CLASSES * 3];
    if ((int)threadIdx.x < n_classes * 3) s_col[threadIdx.x] = colors[threadIdx.x];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (p >= n_pix) return;
    uint32_t nc[MMVAE_PLOT_MAX_CLASSES];
    uint32_t n = 0;
#pragma unroll
    for (int c = 0; c < MMVAE_PLOT_MAX_CLASSES; ++c) {
        nc[c] = c < n_classes ? counts[(size_t)c * n_pix + p] : 0u;
        n += nc[c];  // (a point covers a pixel at most once: n is at most the number of points, < 2^31)
    }
    if (!n) {  // exactly the background, as the host rounded it
        rgba[p] = bg_bytes;
        return;
    }
    float r, g, b;
    {
        const float fn = (float)n;
        float mr = 0.f, mg = 0.f, mb = 0.f;
#pragma unroll
        for (int c = 0; c < MMVAE_PLOT_MAX_CLASSES; ++c) {
            if (c < n_classes) {
                const float w = (float)nc[c] / fn;  // (a true division: exactly 1 for a pixel of one class)
                mr += w * s_col[3 * c], mg += w * s_col[3 * c + 1], mb += w * s_col[3 * c + 2];
            }
        }
        // t = (1 - alpha)^n;  alpha = 1: log2_keep = -inf and t = 0
        const float t = exp2f((float)n * log2_keep), cov = 1.0f - t;
        r = cov * mr + t * bg_r, g = cov * mg + t * bg_g, b = cov * mb + t * bg_b;
    }
    uchar4 out;
    out.x = (unsigned char)fminf(fmaxf(rintf(255.0f * r), 0.f), 255.f);
    out.y = (unsigned char)fminf(fmaxf(rintf(255.0f * g), 0.f), 255.f);
    out.z = (unsigned char)fminf(fmaxf(rintf(255.0f * b), 0.f), 255.f);
    out.w = 255;
    rgba[p] = out;
}

bool raster_ok(int n_classes, int width, int height) {
    return n_classes >= 1 && n_classes <= MMVAE_PLOT_MAX_CLASSES && width >= 1 && width <= MMVAE_PLOT_MAX_SIDE &&
           height >= 1 && height <= MMVAE_PLOT_MAX_SIDE;
}

template <int DIMS, bool PACKED>
int launch_count(bool agg, unsigned groups, hipStream_t st, int64_t n, const float* points, int64_t ld,
                 const int32_t* codes, const View& vw, const Raster& r, uint32_t* counts) {
    if (agg)
        MMVAE_LAUNCH((plot_count_kernel<DIMS, PACKED, true>), dim3(groups), dim3(THREADS), 0, st, n, points, ld, codes, vw,
                     r, counts);
    else
        MMVAE_LAUNCH((plot_count_kernel<DIMS, PACKED, false>), dim3(groups), dim3(THREADS), 0, st, n, points, ld, codes,
                     vw, r, counts);
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}

}  // namespace

extern "C" int mmvae_plot_abi_version(void) { return MMVAE_PLOT_ABI_VERSION; }
extern "C" const char* mmvae_plot_build_arch(void) { return "gfx950"; }

extern "C" int mmvae_plot_count_f32(int64_t n, int dims, const float* points, int64_t ld, const int32_t* codes,
                                    int n_classes, int width, int height, int marker, const float* view_host, int mode,
                                    uint32_t* counts_out, mmvae_stream_t stream) {
    if (n < 1 || n > 0x7fffffff || (dims != 2 && dims != 3) || ld < dims || ld > 0x7fffffff) return MMVAE_ERR_ARG;
    if (!raster_ok(n_classes, width, height) || marker < 1 || marker > MMVAE_PLOT_MAX_MARKER) return MMVAE_ERR_ARG;
    if (mode < MMVAE_PLOT_COUNT_DEFAULT || mode > MMVAE_PLOT_COUNT_AGGREGATE) return MMVAE_ERR_ARG;
    if (!points || !codes || !view_host || !counts_out) return MMVAE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const View vw = {view_host[0], view_host[1], view_host[2], view_host[3],
                     view_host[4], view_host[5], view_host[6], view_host[7]};
    const Raster r = {n_classes, width, height, marker, (marker - 1) / 2, marker / 2};
    const bool agg = mode == MMVAE_PLOT_COUNT_AGGREGATE || (mode == MMVAE_PLOT_COUNT_DEFAULT && DEFAULT_AGG);
    const bool packed = ld == dims && (((uintptr_t)points | (uintptr_t)codes) & 15) == 0;
    (void)hipGetLastError();
    if (hipMemsetAsync(counts_out, 0, (size_t)n_classes * height * width * sizeof(uint32_t), st) != hipSuccess)
        return MMVAE_ERR_LAUNCH;
    const int64_t items = packed ? (n + 3) / 4 : n;  // (n < 4 packed: the loop is empty, workgroup 0 takes the tail)
    const unsigned groups = (unsigned)((items + THREADS - 1) / THREADS < MAX_GROUPS ? (items + THREADS - 1) / THREADS
                                                                                   : MAX_GROUPS);
    if (dims == 2)
        return packed ? launch_count<2, true>(agg, groups, st, n, points, ld, codes, vw, r, counts_out)
                      : launch_count<2, false>(agg, groups, st, n, points, ld, codes, vw, r, counts_out);
    return packed ? launch_count<3, true>(agg, groups, st, n, points, ld, codes, vw, r, counts_out)
                  : launch_count<3, false>(agg, groups, st, n, points, ld, codes, vw, r, counts_out);
}

extern "C" int mmvae_plot_composite_u8(const uint32_t* counts, int n_classes, int width, int height, const float* colors,
                                       float alpha, float bg_r, float bg_g, float bg_b, uint8_t* rgba_out,
                                       mmvae_stream_t stream) {
    if (!raster_ok(n_classes, width, height)) return MMVAE_ERR_ARG;
    if (!(alpha > 0.0f && alpha <= 1.0f)) return MMVAE_ERR_ARG;  // (NaN fails too)
    if (!(bg_r >= 0.0f && bg_r <= 1.0f && bg_g >= 0.0f && bg_g <= 1.0f && bg_b >= 0.0f && bg_b <= 1.0f)) return MMVAE_ERR_ARG;
    if (!counts || !colors || !rgba_out || ((uintptr_t)rgba_out & 3)) return MMVAE_ERR_ARG;
    const int64_t n_pix = (int64_t)width * height;
    const float log2_keep = alpha == 1.0f ? -__builtin_inff() : (float)log2(1.0 - (double)alpha);
    uchar4 bg_bytes;  // rint(255 background) in fp64
    bg_bytes.x = (unsigned char)rint(255.0 * (double)bg_r);
    bg_bytes.y = (unsigned char)rint(255.0 * (double)bg_g);
    bg_bytes.z = (unsigned char)rint(255.0 * (double)bg_b);
    bg_bytes.w = 255;
    MMVAE_LAUNCH(plot_composite_kernel, dim3((unsigned)((n_pix + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                 (hipStream_t)stream, counts, n_classes, n_pix, colors, log2_keep, bg_r, bg_g, bg_b, bg_bytes,
                 reinterpret_cast<uchar4*>(rgba_out));
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
