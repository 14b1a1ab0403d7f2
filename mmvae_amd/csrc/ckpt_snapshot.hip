// The device snapshot behind a checkpoint: copy + checksum + non-finite count of a table of ranges in one launch
// (include/mmvae_ckpt.h) -> libmmvae_ckpt.so.
#include "common.h"
#include "../../include/mmvae_ckpt.h"

namespace {

constexpr int THREADS = 256;
constexpr unsigned CHUNK = MMVAE_CKPT_CHUNK_WORDS;
constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr unsigned EXP_MASK = 0x7F800000u;
typedef unsigned long long u64;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// A source address comes out of the job table, where the compiler cannot see its address space: said here, so that the
// ranges are read with global (not flat) loads.
typedef const unsigned __attribute__((address_space(1))) g_word;
typedef const u32x4 __attribute__((address_space(1))) g_vec;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
    return v;
}

// One word at index j of its chunk: sw += w, swj += w * j (one 32 x 32 + 64 multiply-add), nf += non-finite.
__device__ __forceinline__ void take(unsigned w, unsigned j, u64& sw, u64& swj, unsigned& nf) {
    sw += w;
    swj += (u64)w * j;
    nf += (w & EXP_MASK) == EXP_MASK ? 1u : 0u;
}

// What a workgroup has gathered for one job goes to that job's digest: one 64-bit atomic (two with a non-finite count).
// Called by every thread of the workgroup.
__device__ __forceinline__ void flush(u64 acc, unsigned nf, u64* __restrict__ digest, bool f32) {
    __shared__ u64 sh_acc[THREADS / 64];
    __shared__ unsigned sh_nf[THREADS / 64];
    acc = wave_sum_u64(acc);
    nf = wave_sum_u32(nf);
    if ((threadIdx.x & 63) == 0) {
        sh_acc[threadIdx.x >> 6] = acc;
        sh_nf[threadIdx.x >> 6] = nf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 a = 0;
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            a += sh_acc[w];
            n += sh_nf[w];
        }
        atomicAdd(digest, a * GOLDEN);
        if (f32 && n) atomicAdd(digest + 1, (u64)n);
    }
    __syncthreads();
}

// The work items are (job, chunk) pairs: item = job << lg_cpj | chunk, with 2^lg_cpj >= the chunks of the longest job.  The
// grid is a power of two, and a workgroup walks the items congruent to its index: shifts and masks, no division.  A chunk
// beyond its job's end sends the workgroup straight to its first item of the next job, so the empty part of the item
// space costs one look at the table per job.  Consecutive items of a workgroup mostly belong to one job: its sums stay
// in registers until the job changes, which keeps the atomics on one digest word at one per workgroup.
//
// The checksum, with i = base + j (base: the chunk's first word, j < CHUNK):
//   sum (w_i + 1)(2 i + 1) = sum w_i (2 i + 1) + n^2,    sum_chunk w_i (2 i + 1) = (2 base + 1) sum w + 2 sum w j
// so a word costs one 64-bit add and one 32 x 32 + 64 multiply-add; the multiplication by the golden-ratio constant is
// done once per flush (it distributes over the sum mod 2^64).
template <bool COPY>
__global__ __launch_bounds__(THREADS) void snapshot_kernel(int n_jobs, const mmvae_ckpt_job* __restrict__ jobs, u64 max_words,
                                                           unsigned lg_cpj, unsigned* __restrict__ dst,
                                                           u64* __restrict__ digest) {
    const unsigned tid = threadIdx.x;
    const u64 G = gridDim.x;  // a power of two
    const u64 total = (u64)n_jobs << lg_cpj;
    const u64 chunk_mask = ((u64)1 << lg_cpj) - 1;

    long long cur = -1;  // the job whose sums the registers hold
    bool cur_f32 = false;
    u64 acc = 0;
    unsigned nf = 0;

    for (u64 item = blockIdx.x; item < total;) {
        const u64 job = item >> lg_cpj, chunk = item & chunk_mask;
        const mmvae_ckpt_job J = jobs[job];
        u64 n_words = J.n_words < max_words ? J.n_words : max_words;
        if ((reinterpret_cast<uintptr_t>(J.src) & 3u) != 0) n_words = 0;
        const u64 base = chunk * CHUNK;
        if (base >= n_words) {  // past the job's end: on to this workgroup's first item of the next job
            const u64 nxt = (job + 1) << lg_cpj;
            item = nxt + (((u64)blockIdx.x - nxt) & (G - 1));
            continue;
        }
        if ((long long)job != cur) {
            if (cur >= 0) flush(acc, nf, digest + 2 * cur, cur_f32);
            cur = (long long)job;
            cur_f32 = (J.flags & MMVAE_CKPT_F32) != 0;
            acc = 0;
            nf = 0;
        }
        const unsigned n = (unsigned)(n_words - base < CHUNK ? n_words - base : CHUNK);
        g_word* s = (g_word*)(reinterpret_cast<uintptr_t>(J.src)) + base;
        unsigned* __restrict__ d = COPY ? dst + J.dst_word + base : nullptr;
        const unsigned a_s = (unsigned)(reinterpret_cast<uintptr_t>(s) >> 2) & 3u;
        const bool wide = !COPY || a_s == ((unsigned)(reinterpret_cast<uintptr_t>(d) >> 2) & 3u);

        u64 sw = 0, swj = 0;
        if (wide) {
            const unsigned lead = (4u - a_s) & 3u;
            const unsigned head = lead < n ? lead : n;
            const unsigned nvec = (n - head) >> 2;
            const unsigned edge = n - 4 * nvec;  // head + tail words, < 7
            g_vec* sv = (g_vec*)(s + head);
            u32x4* __restrict__ dv = reinterpret_cast<u32x4*>(d + head);  // (not used when d is null)
            // four 16-byte loads in flight per lane, then their stores, then the arithmetic; a vector past the end is
            // taken as zeros, which add nothing to any of the sums
            for (unsigned v0 = tid; v0 < nvec; v0 += 4 * THREADS) {
                u32x4 w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned v = v0 + k * THREADS;
                    w[k] = sv[v < nvec ? v : nvec - 1];  // (an address inside the chunk; no branch around the load)
                }
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    const unsigned keep = v0 + k * THREADS < nvec ? ~0u : 0u;
                    w[k] &= keep;
                }
                if (COPY) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned v = v0 + k * THREADS;
                        if (v < nvec) dv[v] = w[k];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned j = head + 4 * (v0 + k * THREADS);
                    take(w[k].x, j, sw, swj, nf);
                    take(w[k].y, j + 1, sw, swj, nf);
                    take(w[k].z, j + 2, sw, swj, nf);
                    take(w[k].w, j + 3, sw, swj, nf);
                }
            }
            if (tid < edge) {
                const unsigned j = tid < head ? tid : 4 * nvec + tid;
                const unsigned w = s[j];
                if (COPY) d[j] = w;
                take(w, j, sw, swj, nf);
            }
        } else {
#pragma unroll 4
            for (unsigned j = tid; j < n; j += THREADS) {
                const unsigned w = s[j];
                d[j] = w;
                take(w, j, sw, swj, nf);
            }
        }
        acc += (2 * base + 1) * sw + 2 * swj;
        if (chunk == 0 && tid == 0) acc += n_words * n_words;
        item += G;
    }
    if (cur >= 0) flush(acc, nf, digest + 2 * cur, cur_f32);
}

unsigned ceil_log2(u64 v) {
    unsigned lg = 0;
    while (((u64)1 << lg) < v) ++lg;
    return lg;
}

}  // namespace

extern "C" int mmvae_ckpt_abi_version(void) { return MMVAE_CKPT_ABI_VERSION; }
extern "C" const char* mmvae_ckpt_build_arch(void) { return "gfx950"; }

extern "C" int mmvae_ckpt_check_jobs(int n_jobs, const mmvae_ckpt_job* jobs_host, uint64_t* max_words_out) {
    if (n_jobs < 0 || (!jobs_host && n_jobs > 0)) return MMVAE_ERR_ARG;
    uint64_t most = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const mmvae_ckpt_job& J = jobs_host[j];
        if (reinterpret_cast<uintptr_t>(J.src) & 3u) return MMVAE_ERR_ARG;
        if (!J.src && J.n_words > 0) return MMVAE_ERR_ARG;
        if (J.n_words >> 32) return MMVAE_ERR_ARG;
        if ((J.flags & ~MMVAE_CKPT_F32) || J.reserved) return MMVAE_ERR_ARG;
        if (J.n_words > most) most = J.n_words;
    }
    if (max_words_out) *max_words_out = most;
    return MMVAE_OK;
}

extern "C" int mmvae_ckpt_snapshot(int n_jobs, const mmvae_ckpt_job* jobs_dev, uint64_t max_words, void* dst,
                                   uint64_t* digest, mmvae_stream_t stream) {
    static_assert(sizeof(mmvae_ckpt_job) == 32, "mmvae_ckpt_job is 32 bytes");
    if (n_jobs < 0 || (max_words >> 32)) return MMVAE_ERR_ARG;
    if (n_jobs == 0) return MMVAE_OK;
    if (!jobs_dev || !digest || (reinterpret_cast<uintptr_t>(digest) & 7u)) return MMVAE_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(dst) & 3u) return MMVAE_ERR_ARG;
    (void)hipGetLastError();
    if (hipMemsetAsync(digest, 0, (size_t)n_jobs * 2 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess)
        return MMVAE_ERR_LAUNCH;
    if (max_words == 0) return MMVAE_OK;  // (every range is empty: the cleared digests are the answer)
    const unsigned lg_cpj = ceil_log2((max_words + CHUNK - 1) / CHUNK);
    const u64 total = (u64)n_jobs << lg_cpj;
    const unsigned groups = total >= MMVAE_CKPT_MAX_GROUPS ? MMVAE_CKPT_MAX_GROUPS : 1u << ceil_log2(total);
    if (dst)
        MMVAE_LAUNCH(snapshot_kernel<true>, dim3(groups), dim3(THREADS), 0, (hipStream_t)stream, n_jobs, jobs_dev,
                     (u64)max_words, lg_cpj, static_cast<unsigned*>(dst), reinterpret_cast<u64*>(digest));
    else  // digest only
        MMVAE_LAUNCH(snapshot_kernel<false>, dim3(groups), dim3(THREADS), 0, (hipStream_t)stream, n_jobs, jobs_dev,
                     (u64)max_words, lg_cpj, static_cast<unsigned*>(nullptr), reinterpret_cast<u64*>(digest));
    MMVAE_LAUNCH_CHECK();
    return MMVAE_OK;
}
