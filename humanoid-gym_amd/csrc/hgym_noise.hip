// hgym_noise.hip -- temporally correlated exploration noise (PPO.exploration_noise): the normals of a whole
// rollout, filtered along time, in ONE launch ahead of the rollout.
//
//   noise_table_kernel    hgym_policy_noise_table: z[t][m][j] = carry[t] * state[m][j] + sum_{s <= t} filt[t][s] * w_s[m][j], where w_s[m][j] is
//                         the standard normal the sampling epilogue of a policy launch draws for (env m, action j) at sampling step *step + s
//                         (fwd_body in hgym_fused.hpp, act_sample_kernel in hgym_net.hip: key = seed, counter = (m, step, SLOT_POLICY + j / 4),
//                         Box-Muller on (x, y) and (z, w)).  The sampling epilogues take a row of the table in place of their own draw
//                         (FwdArgs.z), so no existing kernel changes.
//
// Work split.  A "group" is the four normals of one Philox call: (env m, q = j / 4), columns 4 q .. 4 q + 3 of the env's row.  A workgroup owns
// NOISE_GROUPS consecutive groups for all T steps:
//   phase 1   every raw draw of the block, ONE Philox call + two Box-Mullers per (step, group), into LDS as w[s][group] (float4); the lanes
//             also park their group's four state values in registers (they are overwritten at the end)
//   phase 2   wavefront v forms rows t = v, v + 4, ...; lane l owns group l.  The coefficients of row t are the same for every lane: the
//             wavefront loads 64 of them with one coalesced load (lane k holds filt[t][s0 + k]) and hands them out through v_readlane, so the
//             inner loop is one ds_read_b128 and four multiply + add pairs per term -- no Philox call and no global load per term.
// One lane owns a column for all of time, so `state` is read (phase 1) and written (row T - 1, behind the barrier) without a race.
//
// Arithmetic (the contract of include/hgym.h): fp32, x = carry ? carry[t] * state : +0, then x = x + filt[t][s] * w_s for s = 0 .. t, every
// multiply and every add rounded on its own.  This translation unit is built with -ffp-contract=off (build.py); box_muller (hgym_common.hpp)
// gives the same bits under either setting -- its one multiply feeding an add, u01's x * 2^-24, is exact -- so w_s is what the policy
// kernels draw whether they were built contracted (hgym_net.hip) or not (hgym_rollout.hip).
//
// Stores are vector stores: 16 bytes per lane, consecutive lanes consecutive addresses, where A % 4 == 0 and z is 16-byte aligned; element
// by element otherwise (a partial last group of an env's row).
#include "hgym_common.hpp"

namespace hgym {

constexpr int NOISE_THREADS = 256;
constexpr int NOISE_WAVES = NOISE_THREADS / 64;
constexpr int NOISE_GROUPS = 64;      // groups per workgroup = lanes per wavefront: T KiB of LDS (T <= 64: no opt-in; up to 128 KiB of the CU's 160)

struct NoiseArgs {
    int T, A, G;               // steps, actions, groups per env = ceil(A / 4)
    int64_t n, NG;             // envs, groups in all = n * G
    const float* filt;         // (T, ld_filt), lower triangle read
    int64_t ld_filt;
    const float* carry;        // [T] or null
    float* state;              // (n, A) or null (only with carry null)
    uint32_t k0, k1;
    const int64_t* step;
    float* z;                  // (T, n, A)
};

// VEC: A % 4 == 0 and z 16-byte aligned -- every group is whole and leaves as one 16-byte store (an instantiation of its own: with both store
// forms in one kernel the compiler merges their common tails and splits the 16-byte store)
template <bool VEC>
__global__ __launch_bounds__(NOISE_THREADS) void noise_table_kernel(const NoiseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float4 noise_w[];      // [T][NOISE_GROUPS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t g0 = (int64_t)blockIdx.x * NOISE_GROUPS;
    const int T = a.T, A = a.A, G = a.G;
    const int64_t step0 = a.step[0];
    // this lane's group, for both phases (NOISE_THREADS is a multiple of 64: a thread meets one group only); one divide, 32-bit where it can be
    const int64_t g = g0 + lane;
    const bool live = g < a.NG;
    int64_t m = 0;
    if (live) m = a.NG < ((int64_t)1 << 31) ? (int64_t)((uint32_t)g / (uint32_t)G) : g / G;
    const int q = live ? (int)(g - m * G) : 0;
    // ---------------------------------------------------------------- phase 1: the raw draws of this block, once each
    if (live) {
        for (int s = tid >> 6; s < T; s += NOISE_WAVES) {
            const int64_t st = step0 + s;
            const RngKey rk = {a.k0, a.k1, (uint32_t)st, (uint32_t)(st >> 32)};
            const U4 u = rng4(rk, (uint32_t)m, SLOT_POLICY + (uint32_t)q);
            float4 w;
            box_muller(u.x, u.y, w.x, w.y);
            box_muller(u.z, u.w, w.z, w.w);
            noise_w[s * NOISE_GROUPS + lane] = w;
        }
    }
    const int64_t col = m * A + 4 * q;           // this lane's first column of an (n, A) row block
    const int cols = live ? (A - 4 * q < 4 ? A - 4 * q : 4) : 0;
    float x0[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (a.carry) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cols) x0[e] = a.state[col + e];
    }
    __syncthreads();
    // ---------------------------------------------------------------- phase 2: rows t = wave, wave + 4, ...
    const int64_t row_len = a.n * (int64_t)A;
    for (int t = wave; t < T; t += NOISE_WAVES) {
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.carry) {
            const float c = a.carry[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = c * x0[e];
        }
        const float* __restrict__ frow = a.filt + (int64_t)t * a.ld_filt;
        for (int s0 = 0; s0 <= t; s0 += 64) {
            const int cnt = t + 1 - s0 < 64 ? t + 1 - s0 : 64;      // (wave-uniform)
            const int fv = lane < cnt ? __float_as_int(frow[s0 + lane]) : 0;
            // (a lane without a group reads LDS nobody wrote: inside the allocation, never stored)
            const float4* __restrict__ wl = noise_w + s0 * NOISE_GROUPS + lane;
            int k = 0;
            for (; k + 4 <= cnt; k += 4) {      // four LDS reads in flight; the terms still join in ascending s
                float4 w[4];
                float f[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = wl[(k + u) * NOISE_GROUPS];
#pragma unroll
                for (int u = 0; u < 4; ++u) f[u] = __int_as_float(__builtin_amdgcn_readlane(fv, k + u));
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    x[0] = x[0] + f[u] * w[u].x;
                    x[1] = x[1] + f[u] * w[u].y;
                    x[2] = x[2] + f[u] * w[u].z;
                    x[3] = x[3] + f[u] * w[u].w;
                }
            }
            for (; k < cnt; ++k) {
                const float f = __int_as_float(__builtin_amdgcn_readlane(fv, k));
                const float4 w = wl[k * NOISE_GROUPS];
                x[0] = x[0] + f * w.x;
                x[1] = x[1] + f * w.y;
                x[2] = x[2] + f * w.z;
                x[3] = x[3] + f * w.w;
            }
        }
        if (!live) continue;
        float* __restrict__ dst = a.z + (int64_t)t * row_len + col;
        if (VEC) {
            *reinterpret_cast<float4*>(dst) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cols) dst[e] = x[e];
        }
        if (t == T - 1 && a.state) {      // x_{T-1}: where the next rollout's carry term starts
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cols) a.state[col + e] = x[e];
        }
    }
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_policy_noise_table(int32_t T, int64_t n, int32_t A, const float* filt, int64_t ld_filt, const float* carry, float* state,
                                uint64_t seed, const int64_t* step, float* z, void* stream) {
    HG_REQUIRE(T >= 1 && T <= HGYM_NOISE_MAX_STEPS, HGYM_E_SHAPE, "hgym_policy_noise_table: T=%d outside [1, %d]", T, HGYM_NOISE_MAX_STEPS);
    HG_REQUIRE(A >= 1 && A <= HGYM_NUM_ACTIONS, HGYM_E_SHAPE, "hgym_policy_noise_table: A=%d outside [1, %d]", A, HGYM_NUM_ACTIONS);
    HG_REQUIRE(n >= 1, HGYM_E_SHAPE, "hgym_policy_noise_table: n=%lld", (long long)n);
    HG_REQUIRE(filt && step && z, HGYM_E_BADARG, "hgym_policy_noise_table: null filt / step / z");
    HG_REQUIRE(ld_filt >= T, HGYM_E_SHAPE, "hgym_policy_noise_table: ld_filt=%lld below T=%d", (long long)ld_filt, T);
    HG_REQUIRE(!carry || state, HGYM_E_BADARG, "hgym_policy_noise_table: a carry needs the state it multiplies (state is NULL)");
    HG_REQUIRE((((uintptr_t)filt | (uintptr_t)carry | (uintptr_t)state | (uintptr_t)z) & 3) == 0 && ((uintptr_t)step & 7) == 0, HGYM_E_BADARG,
               "hgym_policy_noise_table: filt / carry / state / z must be 4-byte aligned, step 8-byte");
    const int G = (A + 3) / 4;
    HG_REQUIRE(n <= (int64_t)0x7FFFFFFF, HGYM_E_UNSUPPORTED, "hgym_policy_noise_table: n=%lld beyond the 32-bit env word of the draws' counter",
               (long long)n);
    NoiseArgs a;
    a.T = T, a.A = A, a.G = G;
    a.n = n, a.NG = n * G;
    a.filt = filt, a.ld_filt = ld_filt, a.carry = carry, a.state = state;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32);
    a.step = step, a.z = z;
    const bool vec = A % 4 == 0 && ((uintptr_t)z & 15) == 0;
    const void* fn = vec ? reinterpret_cast<const void*>(&noise_table_kernel<true>) : reinterpret_cast<const void*>(&noise_table_kernel<false>);
    const size_t lds = (size_t)T * NOISE_GROUPS * sizeof(float4);
    if (lds > 64 * 1024) {
        const int32_t rc = ensure_dynamic_lds(fn, lds, "noise_table_kernel");
        if (rc) return rc;
    }
    const int64_t blocks = (a.NG + NOISE_GROUPS - 1) / NOISE_GROUPS;
    if (vec) hipLaunchKernelGGL(noise_table_kernel<true>, dim3((unsigned)blocks), dim3(NOISE_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(noise_table_kernel<false>, dim3((unsigned)blocks), dim3(NOISE_THREADS), lds, (hipStream_t)stream, a);
    HG_CHECK_LAUNCH("noise_table_kernel");
    return HGYM_OK;
}

}  // extern "C"
