// hgym_diag.hip -- what a PPO update did to the policy: clip fraction, KL, probability ratios, explained variance (PPO.diagnostics).
//
// A pass of its own BEHIND the update: the rollout storage still holds every row the update trained on (actions, the old mu / sigma /
// log-probability / values, returns, advantages), so the updated nets are evaluated on those rows once more (the forwards the
// configuration already has: hgym_mlp_forward, hgym_critic_values) and one streaming kernel reduces the result.  Nothing of it lives
// inside mlp_fb_kernel or the rollout kernels.
//
// diag_reduce_kernel: one row per lane, 256 rows per workgroup.  The four (M, 12) columns are read as three 16-byte loads per row and
// array (a row is 48 bytes: consecutive lanes consume consecutive bytes, a wavefront 3 KiB per array), the five (M,) columns as one
// float per lane: 212 bytes per row.  The per-row terms are fp32 in the forms of the update's loss head (hgym_fused.hpp, ppo.py:128-166);
// everything summed is widened to fp64 first.
//
// Order of summation, independent of how the caller cuts the rows into calls: lane -> wavefront (shuffle tree) -> workgroup (wavefronts
// 0..3 in turn) -> ONE partial per 256 GLOBAL rows, slot (row0 + i) / 256 of the caller's block; the call with finish = 1 follows with
// a one-workgroup launch that adds the partials in slot order (and takes max / min over them) into the totals.  No atomics at all.
#include <algorithm>

#include "hgym_common.hpp"

namespace hgym {

constexpr int DG_NT = 256;      // rows (= lanes) per workgroup = rows per partial
constexpr int DG_NQ = HGYM_DIAG_SUMS;
static_assert(DG_NT == HGYM_DIAG_ROWS_PER_PARTIAL && DG_NQ == 16 && HGYM_NUM_ACTIONS == 12, "block layout of include/hgym.h");

struct DiagCols {
    const float *actions, *mu_old, *sigma_old, *mu_new;              // (M, 12)
    const float *logp_old, *values_old, *returns, *advantages, *values_new;      // (M,)
    const float* std_;                                               // (12,)
};

__device__ __forceinline__ void load_row12(const float* __restrict__ p, int64_t row, float* out) {
    const float4* __restrict__ q = reinterpret_cast<const float4*>(p + row * 12);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 v = q[k];
        out[4 * k + 0] = v.x; out[4 * k + 1] = v.y; out[4 * k + 2] = v.z; out[4 * k + 3] = v.w;
    }
}

// slots HGYM_DIAG_RATIO_MAX / _MIN combine by max / min, every other one by +
__device__ __forceinline__ double dg_combine(int k, double a, double b) {
    return k == HGYM_DIAG_RATIO_MAX ? fmax(a, b) : (k == HGYM_DIAG_RATIO_MIN ? fmin(a, b) : a + b);
}
__device__ __forceinline__ double dg_identity(int k) {
    return k == HGYM_DIAG_RATIO_MAX ? -__builtin_inf() : (k == HGYM_DIAG_RATIO_MIN ? __builtin_inf() : 0.0);
}

__global__ __launch_bounds__(DG_NT) void diag_reduce_kernel(int64_t M, DiagCols c, float clip, int64_t slot0, double* __restrict__ block) {
    __shared__ double s_q[DG_NT / 64][DG_NQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = (int64_t)blockIdx.x * DG_NT + tid;
    double q[DG_NQ];
#pragma unroll
    for (int k = 0; k < DG_NQ; ++k) q[k] = dg_identity(k);
    if (m < M) {
        float a[12], mo[12], so[12], mn[12];
        load_row12(c.actions, m, a);
        load_row12(c.mu_old, m, mo);
        load_row12(c.sigma_old, m, so);
        load_row12(c.mu_new, m, mn);
        const float lpold = c.logp_old[m], vold = c.values_old[m], ret = c.returns[m], adv = c.advantages[m], vnew = c.values_new[m];
        float lp = 0.0f, ent = 0.0f, kl = 0.0f;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const float s = c.std_[j];
            const float d = a[j] - mn[j];
            lp += -(d * d) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
            ent += 0.5f + 0.9189385332046727f + logf(s);
            // KL(old || new) of the two diagonal Gaussians, exact: the learning-rate rule's expression (ppo.py:138-139) has + 1e-5 inside
            // the logarithm, 12 log(1 + 1e-5) = 1.2e-4 for a policy that has not moved at all
            kl += logf(s / so[j]) + (so[j] * so[j] + (mo[j] - mn[j]) * (mo[j] - mn[j])) / (2.0f * (s * s)) - 0.5f;
        }
        const float dl = lp - lpold;
        const float ratio = expf(dl);
        const float lo = 1.0f - clip, hi = 1.0f + clip;      // as torch.clamp gets them
        const float s1 = -adv * ratio, s2 = -adv * clampf(ratio, lo, hi);
        const float e_old = ret - vold, e_new = ret - vnew;
        q[HGYM_DIAG_COUNT] = 1.0;
        q[HGYM_DIAG_KL] = (double)kl;
        q[HGYM_DIAG_APPROX_KL] = (double)((ratio - 1.0f) - dl);
        q[HGYM_DIAG_RATIO] = (double)ratio;
        q[HGYM_DIAG_CLIPPED] = (ratio < lo || ratio > hi) ? 1.0 : 0.0;
        q[HGYM_DIAG_RATIO_MAX] = (double)ratio;
        q[HGYM_DIAG_RATIO_MIN] = (double)ratio;
        q[HGYM_DIAG_SURROGATE] = (double)fmaxf(s1, s2);
        q[HGYM_DIAG_RET] = (double)ret;
        q[HGYM_DIAG_RET_SQ] = (double)ret * (double)ret;
        q[HGYM_DIAG_ERR_OLD] = (double)e_old;
        q[HGYM_DIAG_ERR_OLD_SQ] = (double)e_old * (double)e_old;
        q[HGYM_DIAG_ERR_NEW] = (double)e_new;
        q[HGYM_DIAG_ERR_NEW_SQ] = (double)e_new * (double)e_new;
        q[HGYM_DIAG_VALUE_CLIPPED] = (fabsf(vnew - vold) > clip) ? 1.0 : 0.0;
        q[HGYM_DIAG_ENTROPY] = (double)ent;
    }
#pragma unroll
    for (int k = 0; k < DG_NQ; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) q[k] = dg_combine(k, q[k], __shfl_down(q[k], off, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DG_NQ; ++k) s_q[wave][k] = q[k];
    }
    __syncthreads();
    if (tid < DG_NQ) {
        double* __restrict__ part = block + HGYM_DIAG_SUMS * (1 + slot0 + (int64_t)blockIdx.x);
        part[tid] = dg_combine(tid, dg_combine(tid, dg_combine(tid, s_q[0][tid], s_q[1][tid]), s_q[2][tid]), s_q[3][tid]);
    }
}

// totals = the P partials combined in slot order.  One workgroup: 256 partials at a time are staged in LDS (coalesced), then lane k
// walks slot k of each in turn -- a chain of dependent fp64 additions, no waiting on memory inside it.
__global__ __launch_bounds__(DG_NT) void diag_finish_kernel(int64_t P, double* __restrict__ block) {
    __shared__ double s_p[DG_NT * DG_NQ];
    const int tid = threadIdx.x;
    const double* __restrict__ part = block + HGYM_DIAG_SUMS;
    double acc = dg_identity(tid & (DG_NQ - 1));
    for (int64_t p0 = 0; p0 < P; p0 += DG_NT) {
        const int n = P - p0 < DG_NT ? (int)(P - p0) : DG_NT;
        for (int i = tid; i < n * DG_NQ; i += DG_NT) s_p[i] = part[p0 * DG_NQ + i];
        __syncthreads();
        if (tid < DG_NQ)
            for (int p = 0; p < n; ++p) acc = dg_combine(tid, acc, s_p[p * DG_NQ + tid]);
        __syncthreads();
    }
    if (tid < DG_NQ) block[tid] = acc;
}

__global__ __launch_bounds__(256) void diag_reset_kernel(int64_t n, double* __restrict__ block) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) block[i] = 0.0;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_ppo_diag_reset(int64_t total_rows, double* block, void* stream) {
    HG_REQUIRE(total_rows >= 0 && total_rows <= HGYM_DIAG_MAX_ROWS && block, HGYM_E_BADARG, "total_rows=%lld, block %p", (long long)total_rows,
               (const void*)block);
    const int64_t count = (int64_t)HGYM_DIAG_BLOCK_DOUBLES(total_rows);
    hipLaunchKernelGGL(diag_reset_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(count, 256), 1024)), dim3(256), 0, (hipStream_t)stream, count,
                       block);
    HG_CHECK_LAUNCH("diag_reset_kernel");
    return HGYM_OK;
}

int32_t hgym_ppo_diag_reduce(int64_t M, const float* actions, const float* mu_old, const float* sigma_old, const float* mu_new,
                             const float* logp_old, const float* values_old, const float* returns, const float* advantages,
                             const float* values_new, const float* std, float clip_param, int64_t row0, int64_t total_rows, int32_t finish,
                             double* block, void* stream) {
    HG_REQUIRE(block && std, HGYM_E_BADARG, "null block / std");
    HG_REQUIRE(finish == 0 || finish == 1, HGYM_E_BADARG, "finish=%d (0 or 1)", finish);
    HG_REQUIRE(M >= 0 && row0 >= 0 && total_rows <= HGYM_DIAG_MAX_ROWS && row0 + M <= total_rows, HGYM_E_BADARG,
               "rows [%lld, %lld + %lld) outside the block's %lld", (long long)row0, (long long)row0, (long long)M, (long long)total_rows);
    HG_REQUIRE(row0 % DG_NT == 0, HGYM_E_BADARG, "row0=%lld is not a multiple of %d", (long long)row0, DG_NT);
    HG_REQUIRE(finish || M % DG_NT == 0, HGYM_E_BADARG, "a call that is not the last must cover a multiple of %d rows, not %lld", DG_NT,
               (long long)M);
    HG_REQUIRE(clip_param >= 0.0f, HGYM_E_BADARG, "clip_param=%g", (double)clip_param);
    if (M > 0) {
        HG_REQUIRE(actions && mu_old && sigma_old && mu_new && logp_old && values_old && returns && advantages && values_new, HGYM_E_BADARG,
                   "null column");
        HG_REQUIRE(aligned16(actions) && aligned16(mu_old) && aligned16(sigma_old) && aligned16(mu_new), HGYM_E_BADARG,
                   "the (M, 12) columns must be 16-byte aligned");
        const DiagCols c = {actions, mu_old, sigma_old, mu_new, logp_old, values_old, returns, advantages, values_new, std};
        hipLaunchKernelGGL(diag_reduce_kernel, dim3((unsigned)ceil_div(M, DG_NT)), dim3(DG_NT), 0, (hipStream_t)stream, M, c, clip_param,
                           row0 / DG_NT, block);
        HG_CHECK_LAUNCH("diag_reduce_kernel");
    }
    if (finish) {
        hipLaunchKernelGGL(diag_finish_kernel, dim3(1), dim3(DG_NT), 0, (hipStream_t)stream, (int64_t)ceil_div(row0 + M, DG_NT), block);
        HG_CHECK_LAUNCH("diag_finish_kernel");
    }
    return HGYM_OK;
}

int32_t hgym_ppo_diagnostics(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* rows, int64_t M,
                             float* scratch, double* block, void* stream) {
    HG_REQUIRE(cfg && ppo && net && rows && block, HGYM_E_BADARG, "null cfg / ppo / net / rows / block");
    HG_REQUIRE(ppo->mirror_coef >= 0.0f && ppo->mirror_coef < INFINITY, HGYM_E_BADARG,
               "HgymPPOConfig.mirror_coef=%g must be finite and >= 0 (0: no mirror loss)", (double)ppo->mirror_coef);      // (a NaN fails it)
    HG_REQUIRE(cfg->num_actions == HGYM_NUM_ACTIONS, HGYM_E_UNSUPPORTED, "num_actions=%d (the reduction reads %d-wide rows)", cfg->num_actions,
               HGYM_NUM_ACTIONS);
    HG_REQUIRE(M >= 0 && M <= HGYM_DIAG_MAX_ROWS, HGYM_E_BADARG, "M=%lld", (long long)M);
    HG_REQUIRE(net->params, HGYM_E_BADARG, "null params");
    if (M > 0) {
        HG_REQUIRE(rows->obs && rows->priv && rows->actions && rows->values && rows->advantages && rows->returns && rows->logp && rows->mu &&
                       rows->sigma && scratch, HGYM_E_BADARG, "null column / scratch");
        HG_REQUIRE(aligned16(scratch), HGYM_E_BADARG, "scratch must be 16-byte aligned");
    }
    const int64_t mb = cfg->max_batch;
    const int64_t piece = M <= mb ? mb : mb / DG_NT * DG_NT;
    HG_REQUIRE(M == 0 || piece > 0, HGYM_E_SHAPE, "M=%lld rows need pieces of a multiple of %d rows; max_batch is %lld", (long long)M, DG_NT,
               (long long)mb);
    float* mu_new = scratch;
    float* v_new = scratch + mb * HGYM_NUM_ACTIONS;
    const float* std = nullptr;      // sigma itself in either HgymNetConfig.std_param mode
    const int32_t rc_std = net_sigma_src(cfg, net, &std);
    if (rc_std) return rc_std;
    if (M == 0)
        return hgym_ppo_diag_reduce(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, std,
                                    ppo->clip_param, 0, 0, 1, block, stream);
    for (int64_t m0 = 0; m0 < M; m0 += piece) {
        const int64_t n = std::min<int64_t>(piece, M - m0);
        int32_t rc = hgym_mlp_forward(cfg, net, 0, (int32_t)n, rows->obs + m0 * cfg->num_obs, cfg->num_obs, mu_new, stream);
        if (rc) return rc;
        rc = hgym_critic_values(cfg, net, n, rows->priv + m0 * cfg->num_priv, v_new, nullptr, stream);
        if (rc) return rc;
        rc = hgym_ppo_diag_reduce(n, rows->actions + m0 * HGYM_NUM_ACTIONS, rows->mu + m0 * HGYM_NUM_ACTIONS,
                                  rows->sigma + m0 * HGYM_NUM_ACTIONS, mu_new, rows->logp + m0, rows->values + m0, rows->returns + m0,
                                  rows->advantages + m0, v_new, std, ppo->clip_param, m0, M, m0 + n >= M ? 1 : 0, block, stream);
        if (rc) return rc;
    }
    return HGYM_OK;
}

}  // extern "C"
