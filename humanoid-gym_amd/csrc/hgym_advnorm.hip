// hgym_advnorm.hip -- hgym_adv_normalize_minibatches: every minibatch's advantages standardised by the minibatch's own statistics
// (PPO.advantage_normalization = "minibatch", rsl_rl's normalize_advantage_per_mini_batch).
//
// update() draws ONE permutation per update and cuts it into num_mini_batches slices that every epoch reuses, so the slices partition the
// drawn rows: one segmented pass per update serves every Adam step.  Segment s = idx[s * seg_len, (s + 1) * seg_len); the pass gathers
// adv[idx[j]], forms the segment's fp64 sum and sum of squares, and scatters (adv - mean) / (std_unbiased + 1e-8) into out[idx[j]] -- a
// second column laid out like the first, which the batch descriptor then names.  Rows no entry names are not touched.
//
// Two launches over the same work items, one per (segment, chunk of ADVMB_CHUNK consecutive entries of the segment; a chunk never
// straddles two segments):
//   adv_mb_sums_kernel   the chunk's partial sums by a fixed tree (lane: entries t, t + 256, ... in that order; lanes, then wavefronts) into
//                        the caller's scratch; the LAST work item of a segment to arrive (a counter per segment in the scratch, left zero
//                        again) adds the segment's partials IN CHUNK ORDER -- gae_kernel's scheme, no fp64 atomics on the sums: the same
//                        bits in every run.
//   adv_mb_apply_kernel  adv_normalize_kernel's arithmetic (hgym_gae.hip, restated: sharing it would rebuild that code object) with the
//                        segment's statistics, gather -> scatter.
// Latency-bound and L2-resident at the workload's shape (245 760 entries: 2 MB of indices read twice, a 1 MB column gathered twice, 1 MB
// scattered; 240 workgroups).  Index reads are coalesced (consecutive lanes, consecutive entries); the gathers and the scatter are not,
// by construction.
#include "hgym_common.hpp"

namespace hgym {

constexpr int ADVMB_THREADS = 256;
constexpr int ADVMB_CHUNK = 1024;                 // entries per work item (hgym.h: the scratch macro's 1024)
constexpr int64_t ADVMB_MAX_BLOCKS = 1 << 16;     // workgroups walk the work items with this stride beyond it
static_assert(HGYM_ADV_MB_SCRATCH_DOUBLES(3, 2 * ADVMB_CHUNK + 1) == 3 * (3 + 2 * 3), "hgym.h's scratch macro and ADVMB_CHUNK disagree");

// scratch: per segment s [3 s] sum, [3 s + 1] sum of squares, [3 s + 2] the arrival counter (its first four bytes); behind the 3 * segments
// doubles the partial sums, two per work item
__global__ __launch_bounds__(ADVMB_THREADS) void adv_mb_sums_kernel(int64_t segments, int64_t seg_len, int64_t chunks, const int64_t* __restrict__ idx,
                                                                    const float* __restrict__ adv, int64_t rows, double* __restrict__ scratch) {
    __shared__ double s_sum[4][2];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* __restrict__ part = scratch + 3 * segments;
    const int64_t items = segments * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t s = item / chunks, k = item - s * chunks;
        const int64_t j0 = k * ADVMB_CHUNK;
        const int n = (int)min((int64_t)ADVMB_CHUNK, seg_len - j0);
        const int64_t* __restrict__ ix = idx + s * seg_len + j0;
        double a = 0.0, b = 0.0;
        for (int e = tid; e < n; e += ADVMB_THREADS) {
            const int64_t r = ix[e];
            if ((uint64_t)r < (uint64_t)rows) {      // the caller's contract; an entry outside the column reads (and writes) nothing
                const double v = (double)adv[r];
                a += v;
                b += v * v;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64);
            b += __shfl_down(b, off, 64);
        }
        if (lane == 0) {
            s_sum[wave][0] = a;
            s_sum[wave][1] = b;
        }
        __syncthreads();
        unsigned int* cnt = reinterpret_cast<unsigned int*>(scratch + 3 * s + 2);
        if (tid == 0) {
            part[2 * item] = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
            part[2 * item + 1] = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const unsigned int done = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (done == (unsigned int)(chunks - 1)) ? 1 : 0;
        }
        __syncthreads();
        if (s_last) {      // (uniform over the workgroup)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const double* p = part + 2 * s * chunks;
            a = 0.0;
            b = 0.0;
            for (int64_t i = tid; i < chunks; i += ADVMB_THREADS) {      // thread t: chunks t, t + 256, ... in that order
                a += p[2 * i];
                b += p[2 * i + 1];
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                a += __shfl_down(a, off, 64);
                b += __shfl_down(b, off, 64);
            }
            if (lane == 0) {
                s_sum[wave][0] = a;
                s_sum[wave][1] = b;
            }
            __syncthreads();
            if (tid == 0) {
                scratch[3 * s] = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
                scratch[3 * s + 1] = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
                __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next call counts from zero
            }
        }
        __syncthreads();      // s_sum and s_last are the next work item's
    }
}

// rollout_storage.py:136 per segment: (adv - mean) / (std_unbiased + 1e-8), mean / std from the fp64 sums, arithmetic in fp32 -- the
// expressions of adv_normalize_kernel, operation for operation (this file is built with -ffp-contract=off as hgym_gae.hip is)
__global__ __launch_bounds__(ADVMB_THREADS) void adv_mb_apply_kernel(int64_t segments, int64_t seg_len, int64_t chunks, const int64_t* __restrict__ idx,
                                                                     const float* __restrict__ adv, float* __restrict__ out, int64_t rows,
                                                                     const double* __restrict__ scratch) {
    const int64_t items = segments * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t s = item / chunks, k = item - s * chunks;
        const int64_t j0 = k * ADVMB_CHUNK;
        const int cn = (int)min((int64_t)ADVMB_CHUNK, seg_len - j0);
        const int64_t* __restrict__ ix = idx + s * seg_len + j0;
        const double n = (double)seg_len;
        const double s0 = scratch[3 * s], s1 = scratch[3 * s + 1];
        const double mean_d = s0 / n;
        double var = (s1 - s0 * s0 / n) / (n - 1.0);
        if (var < 0.0) var = 0.0;
        const float mean = (float)mean_d;
        const float denom = (float)sqrt(var) + 1e-8f;
        for (int e = threadIdx.x; e < cn; e += ADVMB_THREADS) {
            const int64_t r = ix[e];
            if ((uint64_t)r < (uint64_t)rows) out[r] = (adv[r] - mean) / denom;
        }
    }
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_adv_normalize_minibatches(int32_t segments, int64_t seg_len, const int64_t* idx, const float* adv, float* out, int64_t rows,
                                       double* scratch, void* stream) {
    HG_REQUIRE(segments >= 1 && seg_len >= 2, HGYM_E_SHAPE, "segments=%d seg_len=%lld (one value has no unbiased deviation)", segments,
               (long long)seg_len);
    const int64_t limit = (int64_t)1 << 40;
    HG_REQUIRE(seg_len <= limit / segments, HGYM_E_UNSUPPORTED, "segments=%d x seg_len=%lld beyond 2^40 entries", segments, (long long)seg_len);
    HG_REQUIRE(idx && adv && out && scratch, HGYM_E_BADARG, "null pointer");
    const int64_t count = (int64_t)segments * seg_len;
    HG_REQUIRE(rows >= count, HGYM_E_SHAPE, "rows=%lld cannot hold %lld distinct entries", (long long)rows, (long long)count);
    {
        const uintptr_t a0 = (uintptr_t)adv, a1 = a0 + (uintptr_t)rows * 4, o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)rows * 4;
        HG_REQUIRE(a1 <= o0 || o1 <= a0, HGYM_E_BADARG, "adv and out overlap within rows=%lld", (long long)rows);
    }
    const int64_t chunks = (seg_len + ADVMB_CHUNK - 1) / ADVMB_CHUNK;
    const int64_t items = (int64_t)segments * chunks;
    const int blocks = (int)(items < ADVMB_MAX_BLOCKS ? items : ADVMB_MAX_BLOCKS);
    hipLaunchKernelGGL(adv_mb_sums_kernel, dim3(blocks), dim3(ADVMB_THREADS), 0, (hipStream_t)stream, (int64_t)segments, seg_len, chunks, idx, adv,
                       rows, scratch);
    HG_CHECK_LAUNCH("adv_mb_sums_kernel");
    hipLaunchKernelGGL(adv_mb_apply_kernel, dim3(blocks), dim3(ADVMB_THREADS), 0, (hipStream_t)stream, (int64_t)segments, seg_len, chunks, idx, adv,
                       out, rows, (const double*)scratch);
    HG_CHECK_LAUNCH("adv_mb_apply_kernel");
    return HGYM_OK;
}

}  // extern "C"
