// hgym_loss.hpp -- ppo_loss_kernel: the PPO loss head of the layer-by-layer path, one thread per sample.  A header so that its
// instantiations can live in more than one translation unit: hgym_net.hip holds the ones it always had, hgym_loss_mirror.hip the ones with
// the mirror loss (ML) -- inside hgym_net.hip they put that file's device code object past what build.py allows.
#pragma once
#include "hgym_gemm.hpp"
#include "hgym_fused.hpp"

namespace hgym {

// One thread per sample of the minibatch: ppo.py:128-168 forward scalars + the hand-written backward of `loss`
// w.r.t. mu, std and V (oracle/ppo_oracle.py:ppo_loss_and_grads is the executable specification).
struct LossArgs {
    HgymBatch b;
    int A;                       // num_actions
    const float* mu;             // [B][A] current policy mean (fp32 output of the actor)
    const float* val;            // [B]    current value
    const float* std_;           // [A]
    float clip, value_coef, entropy_coef;
    void* dmu;  int64_t ld_dmu;  // [B][Ncp] operand type
    void* dmuT; int64_t ld_t;    // [A16][Mp]
    void* dval; int64_t ld_dval; // [B][Ncp]
    void* dvalT;                 // [16][Mp]
    int Bp;                      // contraction padding of B for this call
    float* partials;             // [gridDim.x][32]: surrogate, value loss, entropy, kl, dstd[12], sum dmu[12], sum dval, pad
    // the mirror loss (ML instantiations; HgymPPOConfig.mirror_coef > 0)
    const float* mt;             // [B][A] raw mu of every row's partner (the pre-pass), rows of the MINIBATCH
    const int32_t* m_src;        // [A] M_a: t_j = m_sign[j] * mt[i][m_src[j]]
    const float* m_sign;         // [A]
    float m_g;                   // 2 * mirror_coef / (B * A)
};

// VU: the unclipped value loss (R - V)^2 (HgymPPOConfig.value_loss_unclipped); a template parameter, so that the clipped kernels stay as
// they were.  ML: the mirror loss (HgymPPOConfig.mirror_coef > 0) -- g (mu - t) joins d mu, (mu - t)^2 the LP_MIRROR partial.  An ML
// instantiation runs BEHIND the plain one on the same arguments and overwrites only what the term changes: d mu (row-major and transposed), the
// LP_DBIAS_MU partials and LP_MIRROR.  Everything else of the minibatch -- d std, d V, the four loss sums -- is what the plain kernel left, the
// same machine code as with the term off, so those bits cannot move (two instantiations of one source need not round alike: the compiler
// contracts multiply-adds per instantiation).
template <typename T, bool VU = false, bool ML = false>
__global__ __launch_bounds__(256) void ppo_loss_kernel(const LossArgs a) {
    __shared__ float red[4][LOSS_PARTIALS];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int B = a.b.B, A = a.A;
    const float invB = 1.0f / (float)B;
    float acc[LOSS_PARTIALS];
#pragma unroll
    for (int k = 0; k < LOSS_PARTIALS; ++k) acc[k] = 0.0f;
    T* dmu = (T*)a.dmu;
    T* dmuT = (T*)a.dmuT;
    T* dval = (T*)a.dval;
    T* dvalT = (T*)a.dvalT;
    if (i < B) {
        const int64_t r = a.b.idx[i];
        const float adv = a.b.advantages[r], ret = a.b.returns[r], vold = a.b.values[r], lpold = a.b.logp[r];
        const float v = a.val[i];
        float lp = 0.0f, ent = 0.0f, kl = 0.0f;
        float diff[16], sg[16];
        // the gathered rows (actions, old mu, old sigma: A floats each, at a random row r) and this sample's mu row.  For the
        // XBot-L width (A = 12: 48-byte rows, 16-byte aligned) they are fetched as three 16-byte loads each: a 4-byte load
        // per element costs the texture path one cache line per lane PER ELEMENT (the rows are scattered), a vector load one
        // per lane per 4 elements -- the kernel was bound by exactly that (31 us for 61 440 samples).
        float rowm[16], rowa[16], rowmo[16], rowso[16];
        if (A == 12) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const float4 qm = reinterpret_cast<const float4*>(a.mu + (int64_t)i * 12)[v];
                const float4 qa = reinterpret_cast<const float4*>(a.b.actions + r * 12)[v];
                const float4 qo = reinterpret_cast<const float4*>(a.b.mu + r * 12)[v];
                const float4 qs = reinterpret_cast<const float4*>(a.b.sigma + r * 12)[v];
                rowm[4 * v] = qm.x; rowm[4 * v + 1] = qm.y; rowm[4 * v + 2] = qm.z; rowm[4 * v + 3] = qm.w;
                rowa[4 * v] = qa.x; rowa[4 * v + 1] = qa.y; rowa[4 * v + 2] = qa.z; rowa[4 * v + 3] = qa.w;
                rowmo[4 * v] = qo.x; rowmo[4 * v + 1] = qo.y; rowmo[4 * v + 2] = qo.z; rowmo[4 * v + 3] = qo.w;
                rowso[4 * v] = qs.x; rowso[4 * v + 1] = qs.y; rowso[4 * v + 2] = qs.z; rowso[4 * v + 3] = qs.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j >= A) continue;
                rowm[j] = a.mu[(int64_t)i * A + j];
                rowa[j] = a.b.actions[r * A + j];
                rowmo[j] = a.b.mu[r * A + j];
                rowso[j] = a.b.sigma[r * A + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            diff[j] = 0.0f;
            sg[j] = 1.0f;
            if (j >= A) continue;
            const float m = rowm[j];
            const float s = m * 0.0f + a.std_[j];
            const float act = rowa[j];
            const float mo = rowmo[j], so = rowso[j];
            const float d = act - m;
            diff[j] = d;
            sg[j] = s;
            lp += -(d * d) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
            ent += 0.5f + 0.9189385332046727f + logf(s);
            kl += logf(s / so + 1.e-5f) + (so * so + (mo - m) * (mo - m)) / (2.0f * (s * s)) - 0.5f;
        }
        const float ratio = expf(lp - lpold);
        const float s1 = -adv * ratio;
        const float s2 = -adv * clampf(ratio, 1.0f - a.clip, 1.0f + a.clip);
        const float surr = fmaxf(s1, s2);
        // backward (torch.max splits ties evenly between its operands; clamp passes gradient on the closed range)
        const float in_range = (ratio >= 1.0f - a.clip && ratio <= 1.0f + a.clip) ? 1.0f : 0.0f;
        const float w1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
        const float d_lp = (-adv) * (w1 + (1.0f - w1) * in_range) * invB * ratio;
        float vl, d_v;
        if constexpr (VU) {         // (R - V)^2: the stored old value plays no part
            vl = (v - ret) * (v - ret);
            d_v = a.value_coef * invB * (2.0f * (v - ret));
        } else {
            const float vc = vold + clampf(v - vold, -a.clip, a.clip);
            const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
            vl = fmaxf(l1, l2);
            const float v_in = ((v - vold) >= -a.clip && (v - vold) <= a.clip) ? 1.0f : 0.0f;
            const float u1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
            d_v = a.value_coef * invB * (u1 * 2.0f * (v - ret) + (1.0f - u1) * 2.0f * (vc - ret) * v_in);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j >= A) continue;
            const float s = sg[j], d = diff[j];
            float g_mu = d_lp * d / (s * s);
            if constexpr (ML) {
                int sj = a.m_src[j];
                sj = sj < 0 ? 0 : (sj >= A ? A - 1 : sj);
                const float dm = rowm[j] - a.m_sign[j] * a.mt[(int64_t)i * A + sj];
                g_mu += a.m_g * dm;
                acc[LP_MIRROR] += dm * dm;
            }
            const float g_sg = d_lp * (d * d / (s * s * s) - 1.0f / s) - (a.entropy_coef * invB) / s;
            if (j < 12) {
                acc[LP_DSTD + j] = g_sg;
                acc[LP_DBIAS_MU + j] = g_mu;
            }
            dmu[(int64_t)i * a.ld_dmu + j] = from_f32<T>(g_mu);
            dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(g_mu);
        }
        if constexpr (!ML) {
            dval[(int64_t)i * a.ld_dval] = from_f32<T>(d_v);
            dvalT[i] = from_f32<T>(d_v);
        }
        acc[LP_SURROGATE] = surr;
        acc[LP_VALUE] = vl;
        acc[LP_ENTROPY] = ent;
        acc[LP_KL] = kl;
        acc[LP_DBIAS_V] = d_v;
    } else if (i < a.Bp) {   // zero the contraction padding of the gradients
        for (int j = 0; j < A; ++j) dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(0.0f);
        if constexpr (!ML) dvalT[i] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int k = 0; k < LOSS_PARTIALS; ++k) {
        float s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if constexpr (ML) {
        const int k = threadIdx.x;
        if ((k >= LP_DBIAS_MU && k < LP_DBIAS_V) || k == LP_MIRROR) a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        return;
    }
    if (threadIdx.x < LOSS_PARTIALS) a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

}  // namespace hgym
