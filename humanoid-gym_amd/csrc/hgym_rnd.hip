// hgym_rnd.hip -- hgym_rnd_rewards: Random Network Distillation's reward pass (rsl_rl's rnd_cfg).
//
// Behind a finished rollout the caller has run the frozen target net and the predictor over the NEXT state of every stored transition;
// this pass turns the two embeddings into the intrinsic reward and adds it to the stored rewards ahead of GAE (include/hgym.h states the
// arithmetic operation by operation; this file is built with -ffp-contract=off so that every operation rounds once, as a test restates it).
//
// Three launches on the caller's stream, no allocation, no host synchronisation, every argument fixed across iterations:
//   rnd_error_kernel  one workgroup per RND_ROWS consecutive rows: the 2 * RND_ROWS * K contiguous floats of the two embeddings are read with
//                     coalesced 16-byte loads (scalar loads for the unaligned tail / an unaligned base), (target - pred)^2 goes through an LDS
//                     tile with an odd row stride, and one lane per row adds the K squares in ascending j -- the order the header promises.
//                     This is the pass's only real traffic: 2 K floats per row.
//   rnd_scan_kernel   one lane per env, the T-loop of the discounted average G in fp64 (coalesced reads of the error column), the rollout's
//                     sum and sum of squares of G by a fixed tree (lanes of the wavefront; workgroups in index order by the LAST workgroup to
//                     arrive -- gae_kernel's scheme, no fp64 atomics), then the merge into the running statistics and std.
//   rnd_apply_kernel  per row of T the weight of the schedule, scale = w / std, intrinsic = err * scale, rewards += intrinsic, and the two
//                     logging sums by the same ordered scheme; the last workgroup advances the step counter.
// Latency-bound at the workload's shape (4096 envs x 60 steps, K = 12: 23.6 MB of embeddings, 5.9 MB of scalar columns; profiles/rnd_cost.txt).
#include "hgym_common.hpp"

namespace hgym {

constexpr int RND_THREADS = 256;
constexpr int RND_ROWS = HGYM_RND_ROWS_PER_WG;        // rows of the error kernel's tile
constexpr int RND_LD = HGYM_RND_MAX_OUTPUTS + 1;      // LDS row stride of the tile at K = the bound (odd: conflict-free column walks)
constexpr int RND_SCAN_ENVS = HGYM_RND_ENVS_PER_PARTIAL;      // envs per workgroup of the scan: ONE wavefront
constexpr int RND_APPLY_WGS = HGYM_RND_APPLY_WGS;     // the apply launch's grid never exceeds the partial slots the block has for it
static_assert(RND_ROWS == 64 && RND_SCAN_ENVS == 64, "one lane per row / env of a 64-lane wavefront");

HG_HD int64_t rnd_part_scan(int64_t n) { return HGYM_RND_HEADER + n; }
HG_HD int64_t rnd_part_apply(int64_t n) { return HGYM_RND_HEADER + n + 2 * ((n + RND_SCAN_ENVS - 1) / RND_SCAN_ENVS); }

// hgym.h: the weight of row t's step count c, in fp64
HG_HD double rnd_weight(const HgymRndConfig& c, int64_t step) {
    if (c.schedule == HGYM_RND_STEP) return step < c.final_step ? c.weight : c.final_value;
    if (c.schedule == HGYM_RND_LINEAR) {
        if (step <= c.initial_step) return c.weight;
        if (step >= c.final_step) return c.final_value;
        return c.weight + (c.final_value - c.weight) * (double)(step - c.initial_step) / (double)(c.final_step - c.initial_step);
    }
    return c.weight;
}

__global__ __launch_bounds__(RND_THREADS) void rnd_block_init_kernel(int64_t doubles, double* __restrict__ block) {
    for (int64_t i = (int64_t)blockIdx.x * RND_THREADS + threadIdx.x; i < doubles; i += (int64_t)gridDim.x * RND_THREADS)
        block[i] = (i == HGYM_RND_VAR) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(RND_THREADS) void rnd_error_kernel(int64_t rows, int K, int vec, const float* __restrict__ pred,
                                                                const float* __restrict__ target, float* __restrict__ err) {
    __shared__ float s_sq[RND_ROWS * RND_LD];
    const int tid = threadIdx.x;
    const int ld = K | 1;
    for (int64_t tile = blockIdx.x; tile * RND_ROWS < rows; tile += gridDim.x) {
        const int64_t r0 = tile * RND_ROWS;
        const int nr = (int)min((int64_t)RND_ROWS, rows - r0);
        const int cnt = nr * K;                                  // contiguous floats of this tile in each embedding
        const float* __restrict__ p = pred + r0 * K;
        const float* __restrict__ q = target + r0 * K;
        const int cnt4 = vec ? (cnt >> 2) : 0;                   // (r0 * K is a multiple of 64 floats: the tile starts as aligned as the base)
        for (int e4 = tid; e4 < cnt4; e4 += RND_THREADS) {
            const float4 a = reinterpret_cast<const float4*>(p)[e4];
            const float4 b = reinterpret_cast<const float4*>(q)[e4];
            const float d[4] = {b.x - a.x, b.y - a.y, b.z - a.z, b.w - a.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = 4 * e4 + u, r = e / K, j = e - r * K;
                s_sq[r * ld + j] = d[u] * d[u];
            }
        }
        for (int e = 4 * cnt4 + tid; e < cnt; e += RND_THREADS) {
            const int r = e / K, j = e - r * K;
            const float d = q[e] - p[e];
            s_sq[r * ld + j] = d * d;
        }
        __syncthreads();
        if (tid < nr) {
            float acc = 0.0f;
            for (int j = 0; j < K; ++j) acc += s_sq[tid * ld + j];
            err[r0 + tid] = (float)sqrt((double)acc);            // the correctly rounded fp32 root: 53 bits >= 2 * 24 + 2
        }
        __syncthreads();                                         // the tile is the next iteration's
    }
}

__global__ __launch_bounds__(RND_SCAN_ENVS) void rnd_scan_kernel(int T, int n, const float* __restrict__ err, HgymRndConfig cfg,
                                                                 double* __restrict__ block) {
    __shared__ int s_last;
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * RND_SCAN_ENVS + lane;
    double* __restrict__ G = block + HGYM_RND_HEADER;
    double* __restrict__ part = block + rnd_part_scan(n);
    double s1 = 0.0, s2 = 0.0;
    if (i < n) {
        double g = G[i];
        int t = 0;
        for (; t + 8 <= T; t += 8) {      // eight independent loads in flight ahead of the serial fp64 chain; the same operations in the same order
            float e[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) e[u] = err[(int64_t)(t + u) * n + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                g = cfg.gamma * g + (double)e[u];
                s1 += g;
                s2 += g * g;
            }
        }
        for (; t < T; ++t) {
            g = cfg.gamma * g + (double)err[(int64_t)t * n + i];
            s1 += g;
            s2 += g * g;
        }
        G[i] = g;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    unsigned int* cnt = reinterpret_cast<unsigned int*>(block + HGYM_RND_TICKET_SCAN);
    if (lane == 0) {
        part[2 * blockIdx.x] = s1;
        part[2 * blockIdx.x + 1] = s2;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned int done = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (done == gridDim.x - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;      // (uniform over the workgroup)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double a = 0.0, b = 0.0;
    for (int w = lane; w < (int)gridDim.x; w += RND_SCAN_ENVS) {      // lane l: workgroups l, l + 64, ... in that order
        a += part[2 * w];
        b += part[2 * w + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    if (lane == 0) {
        // hgym_net_norm_merge's formula with the rollout's T n values as one batch
        const double nb = (double)T * (double)n;
        const double mu_b = a / nb;
        double var_b = b / nb - mu_b * mu_b;
        if (var_b < 0.0) var_b = 0.0;
        double mean = block[HGYM_RND_MEAN], var = block[HGYM_RND_VAR];
        const double count = block[HGYM_RND_COUNT] + nb;
        const double rate = nb / count;
        const double d = mu_b - mean;
        mean += rate * d;
        var += rate * (var_b - var + d * (mu_b - mean));
        block[HGYM_RND_MEAN] = mean;
        block[HGYM_RND_VAR] = var;
        block[HGYM_RND_COUNT] = count;
        block[HGYM_RND_STD] = sqrt(var);
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next call counts from zero
    }
}

__global__ __launch_bounds__(RND_THREADS) void rnd_apply_kernel(int T, int n, int chunks, const float* __restrict__ err, float* __restrict__ rewards,
                                                                float* __restrict__ intrinsic, HgymRndConfig cfg, double* __restrict__ block) {
    __shared__ double s_sum[4][2];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t counter = (int64_t)block[HGYM_RND_COUNTER];
    const double std_d = block[HGYM_RND_STD];
    const bool divide = cfg.normalize != 0 && std_d > 0.0;
    double a = 0.0, b = 0.0;
    const int64_t items = (int64_t)T * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {      // item = (row t, chunk of 256 envs)
        const int t = (int)(item / chunks);
        const int64_t i = (item - (int64_t)t * chunks) * RND_THREADS + tid;
        const double w = rnd_weight(cfg, counter + t + 1);
        const float scale = (float)(divide ? w / std_d : w);
        if (i < n) {
            const int64_t gi = (int64_t)t * n + i;
            const float x = err[gi] * scale;
            const float r = rewards[gi];
            intrinsic[gi] = x;
            rewards[gi] = r + x;
            a += (double)x;
            b += (double)r;
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
    double* __restrict__ part = block + rnd_part_apply(n);
    unsigned int* cnt = reinterpret_cast<unsigned int*>(block + HGYM_RND_TICKET_APPLY);
    if (tid == 0) {
        part[2 * blockIdx.x] = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
        part[2 * blockIdx.x + 1] = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned int done = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (done == gridDim.x - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;      // (uniform over the workgroup)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    a = 0.0;
    b = 0.0;
    for (int w = tid; w < (int)gridDim.x; w += RND_THREADS) {      // thread t: workgroups t, t + 256, ... in that order
        a += part[2 * w];
        b += part[2 * w + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    __syncthreads();      // (every thread has read s_last and the first round's s_sum is used up)
    if (lane == 0) {
        s_sum[wave][0] = a;
        s_sum[wave][1] = b;
    }
    __syncthreads();
    if (tid == 0) {
        block[HGYM_RND_SUM_INTRINSIC] = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
        block[HGYM_RND_SUM_REWARDS] = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
        block[HGYM_RND_WEIGHT_LAST] = rnd_weight(cfg, counter + T);
        block[HGYM_RND_ROWS] = (double)T * (double)n;
        block[HGYM_RND_COUNTER] = (double)(counter + T);      // every workgroup read the counter before it took its ticket
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static bool rnd_weight_ok(double w) { return w >= 0.0 && w <= 1.79769313486231570e308; }      // finite and not negative (NaN fails both)

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_rnd_block_init(int32_t n, double* block, void* stream) {
    HG_REQUIRE(n >= 1 && block, HGYM_E_BADARG, "n=%d block=%p", n, (void*)block);
    const int64_t doubles = (int64_t)HGYM_RND_BLOCK_DOUBLES(n);
    const int blocks = (int)((doubles + RND_THREADS - 1) / RND_THREADS > 1024 ? 1024 : (doubles + RND_THREADS - 1) / RND_THREADS);
    hipLaunchKernelGGL(rnd_block_init_kernel, dim3(blocks), dim3(RND_THREADS), 0, (hipStream_t)stream, doubles, block);
    HG_CHECK_LAUNCH("rnd_block_init_kernel");
    return HGYM_OK;
}

int32_t hgym_rnd_rewards(int32_t T, int32_t n, int32_t K, const float* pred, const float* target, float* rewards, float* err, float* intrinsic,
                         const HgymRndConfig* cfg, double* block, void* stream) {
    HG_REQUIRE(pred && target && rewards && err && intrinsic && cfg && block, HGYM_E_BADARG, "null pointer");
    HG_REQUIRE(T >= 1 && n >= 1 && K >= 1 && K <= HGYM_RND_MAX_OUTPUTS, HGYM_E_BADARG, "T=%d n=%d K=%d (K at most %d)", T, n, K, HGYM_RND_MAX_OUTPUTS);
    HG_REQUIRE(cfg->gamma >= 0.0 && cfg->gamma < 1.0, HGYM_E_BADARG, "gamma=%g outside [0, 1)", cfg->gamma);
    HG_REQUIRE(cfg->schedule == HGYM_RND_CONSTANT || cfg->schedule == HGYM_RND_STEP || cfg->schedule == HGYM_RND_LINEAR, HGYM_E_BADARG,
               "schedule=%d", cfg->schedule);
    HG_REQUIRE(rnd_weight_ok(cfg->weight), HGYM_E_BADARG, "weight=%g: must be finite and >= 0", cfg->weight);
    if (cfg->schedule != HGYM_RND_CONSTANT)
        HG_REQUIRE(rnd_weight_ok(cfg->final_value), HGYM_E_BADARG, "final_value=%g: must be finite and >= 0", cfg->final_value);
    if (cfg->schedule == HGYM_RND_LINEAR)
        HG_REQUIRE(cfg->final_step > cfg->initial_step, HGYM_E_BADARG, "final_step=%lld <= initial_step=%lld", (long long)cfg->final_step,
                   (long long)cfg->initial_step);
    HG_REQUIRE(cfg->normalize == 0 || cfg->normalize == 1, HGYM_E_BADARG, "normalize=%d", cfg->normalize);
    const int64_t rows = (int64_t)T * n;
    const int vec = (((uintptr_t)pred | (uintptr_t)target) & 15) == 0 ? 1 : 0;
    const int64_t tiles = (rows + RND_ROWS - 1) / RND_ROWS;
    hipLaunchKernelGGL(rnd_error_kernel, dim3((unsigned)(tiles < 65536 ? tiles : 65536)), dim3(RND_THREADS), 0, (hipStream_t)stream, rows, (int)K, vec,
                       pred, target, err);
    HG_CHECK_LAUNCH("rnd_error_kernel");
    hipLaunchKernelGGL(rnd_scan_kernel, dim3(ceil_div(n, RND_SCAN_ENVS)), dim3(RND_SCAN_ENVS), 0, (hipStream_t)stream, (int)T, (int)n,
                       (const float*)err, *cfg, block);
    HG_CHECK_LAUNCH("rnd_scan_kernel");
    const int chunks = ceil_div(n, RND_THREADS);
    const int64_t items = (int64_t)T * chunks;
    hipLaunchKernelGGL(rnd_apply_kernel, dim3((unsigned)(items < RND_APPLY_WGS ? items : RND_APPLY_WGS)), dim3(RND_THREADS), 0, (hipStream_t)stream,
                       (int)T, (int)n, chunks, (const float*)err, rewards, intrinsic, *cfg, block);
    HG_CHECK_LAUNCH("rnd_apply_kernel");
    return HGYM_OK;
}

}  // extern "C"
