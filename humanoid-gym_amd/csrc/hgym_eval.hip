// hgym_eval.hip -- the evaluation accumulator: what OnPolicyRunner.evaluate reports, kept on the device and read back once.
//
// One launch behind every vec-step of an evaluation (the fused launch hgym_rollout_eval_step or a plain env step: the kernel reads
// only what both leave behind -- the env state and the step's rew / reset / time_out).  Per step it adds, over all envs: the
// velocity-tracking errors, the reward, and for every env whose episode ended in this step the episode's return and length, whether
// it was a time-out, and the episode sums of the 22 reward terms.
//
// Every sum is fp64 and is formed IN A FIXED ORDER, as the advantage statistics of hgym_gae.hip are: lane -> wavefront (shuffle tree)
// -> workgroup (wavefronts 0..3 in turn) -> per-workgroup partials in the caller's block -> the last workgroup to arrive adds the
// partials in workgroup order onto the totals.  The only atomic is the integer arrival counter.  Two evaluations of the same
// trajectory give the same bits (the fp32 atomics behind extras["episode"] do not: their order varies from run to run).
//
// The episode sums of the reward terms.  The env step adds this step's terms to HgymEnvState::episode_sums and, for an env that
// resets, consumes and zeroes them inside the same launch; no kernel behind the step sees the finished sums.  The accumulator
// therefore keeps a copy of every env's sums as of the PREVIOUS step and credits that copy when the env resets: the per-term sums
// of a finished episode lack the terms of its last step (one step of up to max_episode_length; the episode's return, kept here per
// env from `rew`, does include it).
#include <algorithm>

#include "hgym_common.hpp"

namespace hgym {

constexpr int EV_NT = 256;                         // envs (= lanes) per workgroup
constexpr int EV_NQ = 8 + HGYM_NUM_REWARDS;        // per-env quantities summed per step
static_assert(EV_NQ <= HGYM_EVAL_SUMS - 2 && EV_NT == HGYM_EVAL_ENVS_PER_PARTIAL, "block layout of include/hgym.h");

// quantity q of the per-step sums -> its slot in the block's totals (include/hgym.h: HGYM_EVAL_*)
__device__ __forceinline__ int ev_slot(int q) { return q < 8 ? HGYM_EVAL_ENV_STEPS + q : HGYM_EVAL_TERMS + (q - 8); }

__global__ __launch_bounds__(EV_NT) void eval_accumulate_kernel(int N, const float* __restrict__ commands, const float* __restrict__ lin_vel,
                                                                const float* __restrict__ ang_vel, const float* __restrict__ episode_sums,
                                                                const float* __restrict__ rew, const uint8_t* __restrict__ reset,
                                                                const uint8_t* __restrict__ time_out, double* __restrict__ block) {
    __shared__ double s_q[EV_NT / 64][EV_NQ];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * EV_NT + tid;
    const int P = gridDim.x;
    double* __restrict__ part = block + HGYM_EVAL_SUMS;
    double* __restrict__ cur_ret = part + (int64_t)P * HGYM_EVAL_SUMS;
    double* __restrict__ cur_len = cur_ret + N;
    double* __restrict__ prev_sums = cur_len + N;      // [22][N]
    double q[EV_NQ];
#pragma unroll
    for (int k = 0; k < EV_NQ; ++k) q[k] = 0.0;
    if (e < N) {
        const double dx = (double)commands[e] - (double)lin_vel[e];
        const double dy = (double)commands[N + e] - (double)lin_vel[N + e];
        const double dz = (double)commands[2 * N + e] - (double)ang_vel[2 * N + e];
        const double r = (double)rew[e];
        const bool done = reset[e] != 0;
        const double ret = cur_ret[e] + r, len = cur_len[e] + 1.0;
        q[0] = 1.0;
        q[1] = sqrt(dx * dx + dy * dy);
        q[2] = fabs(dz);
        q[3] = r;
        q[4] = done ? 1.0 : 0.0;
        q[5] = (done && time_out[e] != 0) ? 1.0 : 0.0;
        q[6] = done ? ret : 0.0;
        q[7] = done ? len : 0.0;
        cur_ret[e] = done ? 0.0 : ret;
        cur_len[e] = done ? 0.0 : len;
#pragma unroll
        for (int k = 0; k < HGYM_NUM_REWARDS; ++k) {
            double* ps = prev_sums + (int64_t)k * N + e;
            q[8 + k] = done ? *ps : 0.0;
            *ps = (double)episode_sums[(int64_t)k * N + e];      // (zero again for an env that has just reset)
        }
    }
#pragma unroll
    for (int k = 0; k < EV_NQ; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) q[k] += __shfl_down(q[k], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < EV_NQ; ++k) s_q[wave][k] = q[k];
    }
    __syncthreads();
    if (tid < EV_NQ) part[(int64_t)blockIdx.x * HGYM_EVAL_SUMS + tid] = s_q[0][tid] + s_q[1][tid] + s_q[2][tid] + s_q[3][tid];
    __syncthreads();
    unsigned int* cnt = reinterpret_cast<unsigned int*>(block + HGYM_EVAL_TICKET);
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned int arrived = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (arrived == gridDim.x - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (s_last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (tid < EV_NQ) {
            double a = 0.0;
            for (int b = 0; b < P; ++b) a += part[(int64_t)b * HGYM_EVAL_SUMS + tid];      // workgroups 0, 1, ... in that order
            block[ev_slot(tid)] += a;
        }
        if (tid == 0) {
            block[HGYM_EVAL_STEPS] += 1.0;
            __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next call counts from zero
        }
    }
}

__global__ __launch_bounds__(256) void eval_reset_kernel(int64_t n, double* __restrict__ block) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) block[i] = 0.0;
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_eval_reset(int32_t n, double* block, void* stream) {
    HG_REQUIRE(n > 0 && block, HGYM_E_BADARG, "n=%d, null block", n);
    const int64_t count = (int64_t)HGYM_EVAL_BLOCK_DOUBLES(n);
    hipLaunchKernelGGL(eval_reset_kernel, dim3(std::min<int64_t>(ceil_div(count, 256), 1024)), dim3(256), 0, (hipStream_t)stream, count, block);
    HG_CHECK_LAUNCH("eval_reset_kernel");
    return HGYM_OK;
}

int32_t hgym_eval_accumulate(int32_t n, const float* commands, const float* base_lin_vel, const float* base_ang_vel,
                             const float* episode_sums, const float* rew, const uint8_t* reset, const uint8_t* time_out, double* block,
                             void* stream) {
    HG_REQUIRE(n > 0, HGYM_E_SHAPE, "n=%d", n);
    HG_REQUIRE(commands && base_lin_vel && base_ang_vel && episode_sums && rew && reset && time_out && block, HGYM_E_BADARG, "null pointer");
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(ceil_div(n, EV_NT)), dim3(EV_NT), 0, (hipStream_t)stream, n, commands, base_lin_vel,
                       base_ang_vel, episode_sums, rew, reset, time_out, block);
    HG_CHECK_LAUNCH("eval_accumulate_kernel");
    return HGYM_OK;
}

}  // extern "C"
