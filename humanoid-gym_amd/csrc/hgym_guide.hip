// hgym_guide.hip -- the small kernels of the guidance term (hgym_guide_schedule, hgym_ppo_grad_guide), in a device
// code object of their own so that no existing one changes:
//   guide_schedule_kernel       hgym_guide_schedule: the device-resident update count -> this update's coefficient, count += 1
//   ppo_loss_guide_kernel<T>    the layer-by-layer path's loss head with the teacher's term, fp32 and bf16
//   guide_sums_kernel           the minibatch's squared-error partials -> HgymGuide.sums, in a fixed order
// Host code reaches the last two through launch_ppo_loss_guide and launch_guide_sums only.
#include "hgym_loss.hpp"

namespace hgym {

// hgym.h: the coefficient of update count k, in fp64, left to right (humanoid/algo/ppo/guidance.py: schedule_coef is its twin)
HG_HD double guide_coef(const HgymGuideSchedule& c, int64_t k) {
    if (c.mode == HGYM_GUIDE_STEP) return k < c.final_step ? c.coef : c.final_value;
    if (c.mode == HGYM_GUIDE_LINEAR) {
        if (k <= c.initial_step) return c.coef;
        if (k >= c.final_step) return c.final_value;
        return c.coef + (c.final_value - c.coef) * (double)(k - c.initial_step) / (double)(c.final_step - c.initial_step);
    }
    return c.coef;
}

__global__ __launch_bounds__(64) void guide_schedule_kernel(const HgymGuideSchedule c, int64_t* __restrict__ count, float* __restrict__ coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t k = count[0];
    coef[0] = (float)guide_coef(c, k);      // rounded to fp32 once
    count[0] = k + 1;
}

// Like ppo_loss_smooth_kernel it runs BEHIND the plain ppo_loss_kernel on the same arguments and overwrites only what the term changes:
// d mu (row-major and transposed), the LP_DBIAS_MU partials, and LP_MIRROR with the squared error (a guided minibatch never carries the
// mirror loss).  A kernel of its own and not a parameter of ppo_loss_kernel, for the reason given at ppo_loss_smooth_kernel.
// fp32 operands: d mu_ppo is taken from the d mu the plain kernel left (fp32, exact) -- a second compilation of the same expressions need
// not round alike.  bf16 operands: it is formed here, as in ppo_loss_smooth_kernel.  With the coefficient 0.0 nothing of d mu is written
// at all: the plain kernel's bits stay, only the squared error leaves.
template <typename T>
__global__ __launch_bounds__(256) void ppo_loss_guide_kernel(const LossArgs a, const LossGuide gd) {
    constexpr bool FROM_PLAIN = sizeof(T) == 4;
    __shared__ float red[4][16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int B = a.b.B, A = a.A;
    const float invB = 1.0f / (float)B;
    const float g = gd.coef[0] * gd.inv2;      // a uniform address: one scalar load
    const bool on = g != 0.0f;
    float acc[13];               // [0 .. 12) d mu, [12] |mu - t|^2
#pragma unroll
    for (int k = 0; k < 13; ++k) acc[k] = 0.0f;
    T* dmu = (T*)a.dmu;
    T* dmuT = (T*)a.dmuT;
    if (i < B) {
        const int64_t r = a.b.idx[i];
        float d_lp = 0.0f;
        float diff[16], sg[16], rowm[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            diff[j] = 0.0f;
            sg[j] = 1.0f;
            rowm[j] = 0.0f;
            if (j >= A) continue;
            rowm[j] = a.mu[(int64_t)i * A + j];
        }
        if constexpr (!FROM_PLAIN) {
            const float adv = a.b.advantages[r], lpold = a.b.logp[r];
            float lp = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j >= A) continue;
                const float m = rowm[j];
                const float s = m * 0.0f + a.std_[j];
                const float d = a.b.actions[r * A + j] - m;
                diff[j] = d;
                sg[j] = s;
                lp += -(d * d) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
            }
            const float ratio = expf(lp - lpold);
            const float s1 = -adv * ratio;
            const float s2 = -adv * clampf(ratio, 1.0f - a.clip, 1.0f + a.clip);
            const float in_range = (ratio >= 1.0f - a.clip && ratio <= 1.0f + a.clip) ? 1.0f : 0.0f;
            const float w1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
            d_lp = (-adv) * (w1 + (1.0f - w1) * in_range) * invB * ratio;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j >= A) continue;
            const float s = sg[j], d = diff[j];
            float g_mu = d_lp * d / (s * s);
            if constexpr (FROM_PLAIN) g_mu = to_f32(dmu[(int64_t)i * a.ld_dmu + j]);      // d mu_ppo, as the plain kernel left it
            const float dm = rowm[j] - gd.target[r * A + j];
            g_mu += g * dm;
            acc[12] += dm * dm;
            if (j < 12) acc[j] = g_mu;
            if (on) {
                dmu[(int64_t)i * a.ld_dmu + j] = from_f32<T>(g_mu);
                dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(g_mu);
            }
        }
    }
    // (the contraction padding of the gradient is zero already: the plain kernel wrote it)
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        float s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 13 && (on || k == 12))
        a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + (k < 12 ? LP_DBIAS_MU + k : LP_MIRROR)] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
}

constexpr int GUIDE_SUMS_THREADS = 256;
// One workgroup: thread t adds the LP_MIRROR partial of rows t, t + 256, ... in fp64, ascending; the 256 sums are added in a fixed tree --
// the same bits every run, whatever the device does in between.
__global__ __launch_bounds__(GUIDE_SUMS_THREADS) void guide_sums_kernel(int nblocks, int B, int A, const float* __restrict__ partials,
                                                                        double* __restrict__ sums) {
    __shared__ double red[GUIDE_SUMS_THREADS];
    const int tid = threadIdx.x;
    double se = 0.0;
    for (int b = tid; b < nblocks; b += GUIDE_SUMS_THREADS) se += (double)partials[(int64_t)b * LOSS_PARTIALS + LP_MIRROR];
    red[tid] = se;
    __syncthreads();
    for (int o = GUIDE_SUMS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        sums[0] += red[0] / ((double)B * (double)A);
        sums[1] += 1.0;
    }
}

// (the caller has launched the plain ppo_loss_kernel on `a` just before)
int32_t launch_ppo_loss_guide(const LossArgs& a, const LossGuide& gd, bool bf16, int nblocks, hipStream_t s) {
    if (bf16) hipLaunchKernelGGL((ppo_loss_guide_kernel<__bf16>), dim3(nblocks), dim3(256), 0, s, a, gd);
    else hipLaunchKernelGGL((ppo_loss_guide_kernel<float>), dim3(nblocks), dim3(256), 0, s, a, gd);
    HG_CHECK_LAUNCH("ppo_loss_guide_kernel");
    return HGYM_OK;
}

// the sums of one minibatch of hgym_ppo_grad_guide: partial rows [0, nblocks) of the loss head that has just run
int32_t launch_guide_sums(int nblocks, int B, int A, const float* partials, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(guide_sums_kernel, dim3(1), dim3(GUIDE_SUMS_THREADS), 0, s, nblocks, B, A, partials, sums);
    HG_CHECK_LAUNCH("guide_sums_kernel");
    return HGYM_OK;
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_guide_schedule(const HgymGuideSchedule* sched, int64_t* count, float* coef, void* stream) {
    HG_REQUIRE(sched && count && coef, HGYM_E_BADARG, "hgym_guide_schedule: null sched / count / coef");
    HG_REQUIRE(((uintptr_t)count & 7) == 0 && ((uintptr_t)coef & 3) == 0, HGYM_E_BADARG,
               "hgym_guide_schedule: count must be 8-byte aligned, coef 4-byte");
    HG_REQUIRE(sched->mode == HGYM_GUIDE_CONSTANT || sched->mode == HGYM_GUIDE_STEP || sched->mode == HGYM_GUIDE_LINEAR, HGYM_E_BADARG,
               "hgym_guide_schedule: mode=%d", sched->mode);
    // (written so that a NaN fails it)
    HG_REQUIRE(sched->coef >= 0.0 && sched->coef < (double)INFINITY && sched->final_value >= 0.0 && sched->final_value < (double)INFINITY,
               HGYM_E_BADARG, "hgym_guide_schedule: coef=%g / final_value=%g must be finite and >= 0", sched->coef, sched->final_value);
    if (sched->mode != HGYM_GUIDE_CONSTANT)
        HG_REQUIRE(sched->final_step >= 0, HGYM_E_BADARG, "hgym_guide_schedule: final_step=%lld", (long long)sched->final_step);
    if (sched->mode == HGYM_GUIDE_LINEAR)
        HG_REQUIRE(sched->initial_step >= 0 && sched->final_step > sched->initial_step, HGYM_E_BADARG,
                   "hgym_guide_schedule: final_step=%lld must be greater than initial_step=%lld >= 0", (long long)sched->final_step,
                   (long long)sched->initial_step);
    hipLaunchKernelGGL(guide_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *sched, count, coef);
    HG_CHECK_LAUNCH("guide_schedule_kernel");
    return HGYM_OK;
}

}  // extern "C"
