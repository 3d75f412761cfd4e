// hgym_valnorm.hip -- value-target normalisation by running statistics (PPO.value_normalization; include/hgym.h):
//   hgym_value_denormalize   dst = src * scale_f + mean_f           the critic's outputs -> raw values, ahead of GAE
//   hgym_value_norm_merge    this rollout's raw returns -> (n, mean, var) -> merged into the running (count, mean, var)
//   hgym_value_normalize     x = (x - mean_f) / scale_f in place    returns and old values -> the critic's units, behind the merge
// with mean_f = (float)mean, scale_f = (float)sqrt(var) + eps read from the caller's block of three doubles.  Built with
// -ffp-contract=off: the two maps are two roundings each, as the header states them and as a test restates them in torch fp32.
//
// The statistics.  One work item per chunk of VN_CHUNK consecutive values (a workgroup of 256 threads, four values a thread, one 16-byte
// load where the column is 16-byte aligned): the chunk's (mean, M2 = sum (x - mean)^2) in fp64, TWO PASSES over the registers, each a
// fixed tree (thread: its values in order; lanes: __shfl_down 32 .. 1; wavefronts 0 .. 3 in order).  The chunk's mean is near every
// value of the chunk, so x - mean is exact or nearly so whatever |mean| / std of the column is -- no sum of squares of raw values is ever
// formed.  The partials go to the caller's scratch; the LAST work item to arrive (a counter in the scratch, left zero again:
// adv_mb_sums_kernel's scheme, no fp64 atomics) combines them by Chan's pairwise rule in a fixed order (thread t: chunks t, t + 256, ...
// in that order; lanes; wavefronts), leaves the batch's raw (n, mean, var) in scratch[0 .. 2] and merges them into the block: the same
// bits in every run.  The three kernels are latency-bound at the workload's shape (245 760 values, 1 MB: 240 workgroups each).
#include "hgym_common.hpp"

namespace hgym {

constexpr int VN_THREADS = 256;
constexpr int VN_CHUNK = 1024;              // values per work item (hgym.h: HGYM_VALUE_NORM_CHUNK)
constexpr int VN_MAX_BLOCKS = 1024;         // workgroups walk the chunks with this stride beyond it (hgym.h: HGYM_VALUE_NORM_MAX_BLOCKS)
static_assert(VN_CHUNK == HGYM_VALUE_NORM_CHUNK && VN_MAX_BLOCKS == HGYM_VALUE_NORM_MAX_BLOCKS && VN_CHUNK == 4 * VN_THREADS, "hgym.h and hgym_valnorm.hip disagree");
static_assert(HGYM_VALUE_NORM_SCRATCH_DOUBLES(2 * VN_CHUNK + 1) == HGYM_VALUE_NORM_PARTIALS + 2 * 3, "hgym.h's scratch macro and VN_CHUNK disagree");

struct VnStat {      // n values of mean `mean` with sum of squared deviations m2
    double n, mean, m2;
};

// Chan, Golub, LeVeque: the statistics of a followed by b
__device__ __forceinline__ VnStat vn_combine(const VnStat& a, const VnStat& b) {
    if (!(b.n > 0.0)) return a;
    if (!(a.n > 0.0)) return b;
    VnStat r;
    r.n = a.n + b.n;
    const double d = b.mean - a.mean;
    r.mean = a.mean + d * (b.n / r.n);
    r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / r.n);
    return r;
}

__device__ __forceinline__ VnStat vn_shfl_down(const VnStat& s, int off) {
    VnStat r;
    r.n = __shfl_down(s.n, off, 64);
    r.mean = __shfl_down(s.mean, off, 64);
    r.m2 = __shfl_down(s.m2, off, 64);
    return r;
}

// the up to four values of thread `tid` of the chunk at x0 (cn values): v[0 .. k)
__device__ __forceinline__ int vn_load4(const float* __restrict__ x0, int cn, int tid, int vec, float v[4]) {
    const int e = 4 * tid;
    const int k = min(4, max(0, cn - e));
    if (vec && k == 4) {
        const float4 q = *reinterpret_cast<const float4*>(x0 + e);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        for (int i = 0; i < 4; ++i) v[i] = i < k ? x0[e + i] : 0.0f;
    }
    return k;
}

__global__ __launch_bounds__(VN_THREADS) void value_norm_merge_kernel(int64_t n, int64_t chunks, const float* __restrict__ x, int vec,
                                                                      double* __restrict__ block, double* __restrict__ scratch) {
    __shared__ double s_sum[4];
    __shared__ double s_tri[4][3];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* __restrict__ part = scratch + HGYM_VALUE_NORM_PARTIALS;
    unsigned int* cnt = reinterpret_cast<unsigned int*>(scratch + HGYM_VALUE_NORM_TICKET);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t j0 = c * VN_CHUNK;
        const int cn = (int)min((int64_t)VN_CHUNK, n - j0);
        float v[4];
        const int k = vn_load4(x + j0, cn, tid, vec, v);
        // pass 1: the chunk's mean
        double a = 0.0;
        for (int i = 0; i < k; ++i) a += (double)v[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) s_sum[wave] = a;
        __syncthreads();
        const double mean_c = (s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]) / (double)cn;      // (every thread: the same expression, the same bits)
        __syncthreads();
        // pass 2: the squared deviations from it
        double b = 0.0;
        for (int i = 0; i < k; ++i) {
            const double d = (double)v[i] - mean_c;
            b += d * d;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) b += __shfl_down(b, off, 64);
        if (lane == 0) s_sum[wave] = b;
        __syncthreads();
        if (tid == 0) {
            part[2 * c] = mean_c;
            part[2 * c + 1] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const unsigned int done = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (done == (unsigned int)(chunks - 1)) ? 1 : 0;
        }
        __syncthreads();
        if (s_last) {      // (uniform over the workgroup)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            VnStat acc = {0.0, 0.0, 0.0};
            for (int64_t i = tid; i < chunks; i += VN_THREADS) {      // thread t: chunks t, t + 256, ... in that order
                const VnStat p = {(double)min((int64_t)VN_CHUNK, n - i * VN_CHUNK), part[2 * i], part[2 * i + 1]};
                acc = vn_combine(acc, p);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const VnStat o = vn_shfl_down(acc, off);
                if (lane + off < 64) acc = vn_combine(acc, o);
            }
            if (lane == 0) {
                s_tri[wave][0] = acc.n;
                s_tri[wave][1] = acc.mean;
                s_tri[wave][2] = acc.m2;
            }
            __syncthreads();
            if (tid == 0) {
                VnStat t = {s_tri[0][0], s_tri[0][1], s_tri[0][2]};
                for (int w = 1; w < 4; ++w) t = vn_combine(t, VnStat{s_tri[w][0], s_tri[w][1], s_tri[w][2]});
                const double nb = t.n, mean_b = t.mean;
                double var_b = t.m2 / nb;
                if (!(var_b > 0.0)) var_b = 0.0;
                scratch[HGYM_VALUE_NORM_BATCH] = nb;
                scratch[HGYM_VALUE_NORM_BATCH + 1] = mean_b;
                scratch[HGYM_VALUE_NORM_BATCH + 2] = var_b;
                // norm_merge_kernel's merge (hgym_norm.hip); from count = 0 its value is the batch's statistics themselves
                const double count = block[0], mean = block[1], var = block[2];
                const double count_new = count + nb;
                if (!(count > 0.0)) {
                    block[1] = mean_b;
                    block[2] = var_b;
                } else {
                    const double rate = nb / count_new;
                    const double d = mean_b - mean;
                    const double mean_new = mean + rate * d;
                    double var_new = var + rate * (var_b - var + d * (mean_b - mean_new));
                    if (!(var_new > 0.0)) var_new = 0.0;
                    block[1] = mean_new;
                    block[2] = var_new;
                }
                block[0] = count_new;
                __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next call counts from zero
            }
        }
        __syncthreads();      // s_sum, s_tri and s_last are the next chunk's
    }
}

// NORM: y = (x - mean_f) / scale_f, else V = v * scale_f + mean_f; two fp32 roundings each.  src == dst is fine: a thread reads its
// values before it writes them and nobody else touches them.
template <bool NORM>
__global__ __launch_bounds__(VN_THREADS) void value_map_kernel(int64_t n, int64_t chunks, const float* src, float* dst, int vec,
                                                               const double* __restrict__ block, float eps) {
    const float mean_f = (float)block[1];
    const float scale_f = (float)sqrt(block[2]) + eps;
    const int tid = threadIdx.x;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t j0 = c * VN_CHUNK + 4 * tid;
        const int k = (int)min((int64_t)4, max((int64_t)0, n - j0));
        if (vec && k == 4) {
            float4 q = *reinterpret_cast<const float4*>(src + j0);
            if (NORM) {
                q.x = (q.x - mean_f) / scale_f, q.y = (q.y - mean_f) / scale_f, q.z = (q.z - mean_f) / scale_f, q.w = (q.w - mean_f) / scale_f;
            } else {
                q.x = q.x * scale_f + mean_f, q.y = q.y * scale_f + mean_f, q.z = q.z * scale_f + mean_f, q.w = q.w * scale_f + mean_f;
            }
            *reinterpret_cast<float4*>(dst + j0) = q;
        } else {
            for (int i = 0; i < k; ++i) {
                const float xv = src[j0 + i];
                dst[j0 + i] = NORM ? (xv - mean_f) / scale_f : xv * scale_f + mean_f;
            }
        }
    }
}

static int32_t vn_check(int64_t n, const void* block, float eps, bool with_eps) {
    HG_REQUIRE(n >= 1, HGYM_E_SHAPE, "n=%lld", (long long)n);
    HG_REQUIRE(n <= ((int64_t)1 << 40), HGYM_E_UNSUPPORTED, "n=%lld beyond 2^40 values", (long long)n);
    HG_REQUIRE(block, HGYM_E_BADARG, "null block");
    HG_REQUIRE((uintptr_t)block % 8 == 0, HGYM_E_BADARG, "block is not 8-byte aligned");
    if (with_eps) HG_REQUIRE(__builtin_isfinite(eps) && eps >= 0.0f, HGYM_E_BADARG, "eps=%g: must be finite and >= 0", (double)eps);
    return HGYM_OK;
}

static inline int vn_blocks(int64_t chunks) { return (int)(chunks < VN_MAX_BLOCKS ? chunks : VN_MAX_BLOCKS); }

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_value_denormalize(int64_t n, const float* src, float* dst, const double* block, float eps, void* stream) {
    const int32_t rc = vn_check(n, block, eps, true);
    if (rc) return rc;
    HG_REQUIRE(src && dst, HGYM_E_BADARG, "null pointer");
    HG_REQUIRE((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0, HGYM_E_BADARG, "src / dst not 4-byte aligned");
    if (src != dst) {
        const uintptr_t a0 = (uintptr_t)src, a1 = a0 + (uintptr_t)n * 4, o0 = (uintptr_t)dst, o1 = o0 + (uintptr_t)n * 4;
        HG_REQUIRE(a1 <= o0 || o1 <= a0, HGYM_E_BADARG, "src and dst overlap without being the same column");
    }
    const int64_t chunks = (n + VN_CHUNK - 1) / VN_CHUNK;
    const int vec = (((uintptr_t)src | (uintptr_t)dst) % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(value_map_kernel<false>, dim3(vn_blocks(chunks)), dim3(VN_THREADS), 0, (hipStream_t)stream, n, chunks, src, dst, vec, block, eps);
    HG_CHECK_LAUNCH("value_map_kernel<denormalize>");
    return HGYM_OK;
}

int32_t hgym_value_normalize(int64_t n, float* x, const double* block, float eps, void* stream) {
    const int32_t rc = vn_check(n, block, eps, true);
    if (rc) return rc;
    HG_REQUIRE(x, HGYM_E_BADARG, "null pointer");
    HG_REQUIRE((uintptr_t)x % 4 == 0, HGYM_E_BADARG, "x not 4-byte aligned");
    const int64_t chunks = (n + VN_CHUNK - 1) / VN_CHUNK;
    const int vec = ((uintptr_t)x % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(value_map_kernel<true>, dim3(vn_blocks(chunks)), dim3(VN_THREADS), 0, (hipStream_t)stream, n, chunks, (const float*)x, x, vec, block,
                       eps);
    HG_CHECK_LAUNCH("value_map_kernel<normalize>");
    return HGYM_OK;
}

int32_t hgym_value_norm_merge(int64_t n, const float* returns, double* block, double* scratch, void* stream) {
    const int32_t rc = vn_check(n, block, 0.0f, false);
    if (rc) return rc;
    HG_REQUIRE(returns && scratch, HGYM_E_BADARG, "null pointer");
    HG_REQUIRE((uintptr_t)returns % 4 == 0, HGYM_E_BADARG, "returns not 4-byte aligned");
    HG_REQUIRE((uintptr_t)scratch % 8 == 0, HGYM_E_BADARG, "scratch is not 8-byte aligned");
    const int64_t chunks = (n + VN_CHUNK - 1) / VN_CHUNK;
    const int vec = ((uintptr_t)returns % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(value_norm_merge_kernel, dim3(vn_blocks(chunks)), dim3(VN_THREADS), 0, (hipStream_t)stream, n, chunks, returns, vec, block, scratch);
    HG_CHECK_LAUNCH("value_norm_merge_kernel");
    return HGYM_OK;
}

}  // extern "C"
