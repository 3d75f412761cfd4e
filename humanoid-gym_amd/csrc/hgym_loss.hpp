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

// ------------------------------------------------------------------------------------------------ smoothness (hgym_ppo_grad_smooth)
// ppo_loss_smooth_kernel: the layer-by-layer path's head with the smoothness regulariser.  Like an ML instantiation it runs BEHIND the plain
// ppo_loss_kernel on the same arguments and overwrites only what the terms change: d mu (row-major and transposed), the LP_DBIAS_MU
// partials, and the two squared-error partials LP_SMOOTH_T / LP_SMOOTH_S.  A kernel of its own and not one more template parameter of
// ppo_loss_kernel: a parameter would rename every existing instantiation, and LossArgs -- their kernel argument -- keeps its layout.  The
// value-loss form does not enter (d V is the plain kernel's).  A term whose g is 0 is off and its pointers are not read.
struct LossSmooth {
    const float* tnext;          // [B][A] mu of every row's successor (the temporal pre-pass), rows of the MINIBATCH
    const float* tnear;          // [B][A] mu of every row's perturbed copy (the spatial pre-pass)
    const float* weight;         // [B] 0 where the row has no successor, else 1
    float gT, gS;                // 2 * coef / (B * A)
};

template <typename T>
__global__ __launch_bounds__(256) void ppo_loss_smooth_kernel(const LossArgs a, const LossSmooth sm) {
    __shared__ float red[4][16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int B = a.b.B, A = a.A;
    const float invB = 1.0f / (float)B;
    float acc[14];               // [0 .. 12) d mu, [12] w |mu - tnext|^2, [13] |mu - tnear|^2
#pragma unroll
    for (int k = 0; k < 14; ++k) acc[k] = 0.0f;
    T* dmu = (T*)a.dmu;
    T* dmuT = (T*)a.dmuT;
    const bool onT = sm.gT > 0.0f, onS = sm.gS > 0.0f;
    if (i < B) {
        const int64_t r = a.b.idx[i];
        const float adv = a.b.advantages[r], lpold = a.b.logp[r];
        float lp = 0.0f;
        float diff[16], sg[16], rowm[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            diff[j] = 0.0f;
            sg[j] = 1.0f;
            rowm[j] = 0.0f;
            if (j >= A) continue;
            const float m = a.mu[(int64_t)i * A + j];
            const float s = m * 0.0f + a.std_[j];
            const float d = a.b.actions[r * A + j] - m;
            rowm[j] = m;
            diff[j] = d;
            sg[j] = s;
            lp += -(d * d) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
        }
        const float ratio = expf(lp - lpold);
        const float s1 = -adv * ratio;
        const float s2 = -adv * clampf(ratio, 1.0f - a.clip, 1.0f + a.clip);
        const float in_range = (ratio >= 1.0f - a.clip && ratio <= 1.0f + a.clip) ? 1.0f : 0.0f;
        const float w1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
        const float d_lp = (-adv) * (w1 + (1.0f - w1) * in_range) * invB * ratio;
        const float wgt = onT ? sm.weight[i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j >= A) continue;
            const float s = sg[j], d = diff[j];
            float g_mu = d_lp * d / (s * s);
            if (onT) {
                const float dm = rowm[j] - sm.tnext[(int64_t)i * A + j];
                g_mu += sm.gT * wgt * dm;
                acc[12] += wgt * dm * dm;
            }
            if (onS) {
                const float dm = rowm[j] - sm.tnear[(int64_t)i * A + j];
                g_mu += sm.gS * dm;
                acc[13] += dm * dm;
            }
            if (j < 12) acc[j] = g_mu;
            dmu[(int64_t)i * a.ld_dmu + j] = from_f32<T>(g_mu);
            dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(g_mu);
        }
    } else if (i < a.Bp) {       // the contraction padding of the gradient stays zero
        for (int j = 0; j < A; ++j) dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int k = 0; k < 14; ++k) {
        float s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 14) a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + (k < 12 ? LP_DBIAS_MU + k : LP_SMOOTH_T + (k - 12))] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
}

// ------------------------------------------------------------------------------------------------ guidance (hgym_ppo_grad_guide)
// The argument of ppo_loss_guide_kernel (hgym_guide.hip), the layer-by-layer path's head with the frozen teacher's cloning term.
struct LossGuide {
    const float* target;         // (num_rows, A) the teacher's mean of every stored row, gathered through idx
    const float* coef;           // one device float: this update's coefficient
    float inv2;                  // 2 / (B * A)
};

// ------------------------------------------------------------------------------------------------ behaviour cloning (hgym_bc_grad)
// bc_loss_kernel: the regression head of the layer-by-layer path, one thread per sample: e = mu - target[idx[i]], d mu into the actor's
// last dY / dYT (the operands of the backward that follows), the sample's loss terms and d mu into the block's partial row (LP_MIRROR --
// the partial row's regression slot -- and LP_DBIAS_MU).  bc_scalars_kernel: one workgroup that adds the partial rows of either path in a
// fixed order (16 interleaved fp64 sums per quantity, as ppo_scalars_block) -> sums[0] += loss, sums[1] += 1, opt[HGYM_OPT_GRAD_SQNORM] = 0
// for the slab sum behind it, and -- fused path -- the head bias gradient.  It touches no other slot of opt_state.
struct BcLossArgs {
    const float* mu;             // [B][A] the actor's fp32 output
    const float* target;         // (num_rows, A), gathered through idx
    const int64_t* idx;
    int B, Bp, A;
    void* dmu;  int64_t ld_dmu;  // [B][Ncp] operand type
    void* dmuT; int64_t ld_t;    // [A16][Mp]
    float inv, delta;            // 1 / (B A); Huber's delta
    int huber;
    float* partials;             // [gridDim.x][LOSS_PARTIALS]
};
struct BcScalArgs {
    int nblocks, B, A;
    const float* partials;
    float* grads_bmu;            // the head bias gradient (fused path), null: it comes from the slabs
    double* opt;
    double* sums;
};

template <typename T>
__global__ __launch_bounds__(256) void bc_loss_kernel(const BcLossArgs a) {
    __shared__ float red[4][16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int A = a.A;
    float acc[13];               // [0 .. 12) d mu, [12] the loss terms
#pragma unroll
    for (int k = 0; k < 13; ++k) acc[k] = 0.0f;
    T* dmu = (T*)a.dmu;
    T* dmuT = (T*)a.dmuT;
    if (i < a.B) {
        const int64_t r = a.idx[i];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            if (j >= A) continue;
            const float d = a.mu[(int64_t)i * A + j] - a.target[r * A + j];
            float gd, le;
            if (a.huber) {
                const float ad = fabsf(d);
                gd = clampf(d, -a.delta, a.delta);
                le = ad <= a.delta ? 0.5f * d * d : a.delta * (ad - 0.5f * a.delta);
            } else {
                gd = 2.0f * d;
                le = d * d;
            }
            const float g = gd * a.inv;
            acc[j] = g;
            acc[12] += le;
            dmu[(int64_t)i * a.ld_dmu + j] = from_f32<T>(g);
            dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(g);
        }
    } else if (i < a.Bp) {       // zero the contraction padding of the gradient
        for (int j = 0; j < A; ++j) dmuT[(int64_t)j * a.ld_t + i] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        float s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 13) a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + (k < 12 ? LP_DBIAS_MU + k : LP_MIRROR)] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
}

template <int THREADS = 512>      // (a template: emitted only where it is launched, hgym_update_bc.hip)
__global__ __launch_bounds__(THREADS) void bc_scalars_kernel(const BcScalArgs a) {
    static_assert(THREADS == 16 * LOSS_PARTIALS, "16 partial sums per quantity");
    __shared__ double red[16][LOSS_PARTIALS + 1];
    const int tid = threadIdx.x;
    const int k = tid & (LOSS_PARTIALS - 1), part = tid / LOSS_PARTIALS;      // 512 threads: 16 parts
    const bool used = (k >= LP_DBIAS_MU && k < LP_DBIAS_V) || k == LP_MIRROR;
    double s = 0.0;
    if (used)
        for (int b = part; b < a.nblocks; b += 16) s += (double)a.partials[(int64_t)b * LOSS_PARTIALS + k];
    red[part][k] = s;
    __syncthreads();
    if (tid < LOSS_PARTIALS && used) {
        double t = 0.0;
        for (int p = 0; p < 16; ++p) t += red[p][tid];
        if (tid == LP_MIRROR) {
            a.sums[0] += t / ((double)a.B * (double)a.A);
            a.sums[1] += 1.0;
            a.opt[HGYM_OPT_GRAD_SQNORM] = 0.0;      // accumulated by reduce_slabs_kernel later in this call
        } else if (a.grads_bmu && tid - LP_DBIAS_MU < a.A) {
            a.grads_bmu[tid - LP_DBIAS_MU] = (float)t;
        }
    }
}

// ------------------------------------------------------------------------------------------------ critic only (hgym_vf_grad, hgym_bc_vf_grad)
// vf_loss_kernel: the value part of ppo_loss_kernel alone, the layer-by-layer path's head of a critic-only step, one thread per sample:
// d V into the critic's last dY / dYT (the operands of the backward that follows), zero in the contraction padding, and the block's two
// partials LP_VALUE / LP_DBIAS_V -- no other slot of the partial row is written, so a cloning head's row (LP_DBIAS_MU, LP_MIRROR) may share it.
// vf_scalars_kernel: one workgroup that adds the partial rows of either path -- LP_VALUE and LP_DBIAS_V in ppo_scalars_block's order (16
// interleaved fp64 sums per quantity, each of four chains combined as (s0 + s1) + (s2 + s3)), so that the critic's head bias gradient has
// the bits hgym_ppo_grad gives it -> sums[0] += the mean value loss, sums[1] += 1, the head bias gradient (fused path), and
// opt[HGYM_OPT_GRAD_SQNORM] = 0 unless the caller keeps what is there.  With bc_sums set it is also bc_scalars_kernel, quantity by
// quantity in that kernel's own order: the one scalars workgroup of hgym_bc_vf_grad.  It touches no other slot of opt_state.
struct VfLossArgs {
    const float* val;            // [B] the critic's fp32 output
    const float* values;         // (num_rows,) the stored old values, gathered through idx; not read by the unclipped form
    const float* returns;        // (num_rows,)
    const int64_t* idx;
    int B, Bp;
    void* dval; int64_t ld_dval; // [B][Ncp] operand type
    void* dvalT;                 // [16][Mp]
    float clip, value_coef;
    float* partials;             // [gridDim.x][LOSS_PARTIALS]
};
struct VfScalArgs {
    int nblocks, B, A;
    const float* partials;
    float* grads_bv;             // the critic's head bias gradient (fused path), null: it comes from the slabs
    double* opt;
    double* sums;                // the value loss's two sums
    int keep_sqnorm;             // 1: opt[HGYM_OPT_GRAD_SQNORM] is left as found (the slab sum behind adds to it)
    float* grads_bmu;            // with bc_sums: the actor's head bias gradient (fused path), null: it comes from the slabs
    double* bc_sums;             // non-null: the cloning loss's two sums, as bc_scalars_kernel leaves them
};

template <typename T, bool VU>
__global__ __launch_bounds__(256) void vf_loss_kernel(const VfLossArgs a) {
    __shared__ float red[4][2];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float invB = 1.0f / (float)a.B;
    float vl = 0.0f, d_v = 0.0f;
    T* dval = (T*)a.dval;
    T* dvalT = (T*)a.dvalT;
    if (i < a.B) {
        const int64_t r = a.idx[i];
        const float ret = a.returns[r];
        const float v = a.val[i];
        if constexpr (VU) {         // (R - V)^2: the stored old value plays no part
            vl = (v - ret) * (v - ret);
            d_v = a.value_coef * invB * (2.0f * (v - ret));
        } else {
            const float vold = a.values[r];
            const float vc = vold + clampf(v - vold, -a.clip, a.clip);
            const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
            vl = fmaxf(l1, l2);
            // backward (torch.max splits ties evenly between its operands; clamp passes gradient on the closed range)
            const float v_in = ((v - vold) >= -a.clip && (v - vold) <= a.clip) ? 1.0f : 0.0f;
            const float u1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
            d_v = a.value_coef * invB * (u1 * 2.0f * (v - ret) + (1.0f - u1) * 2.0f * (vc - ret) * v_in);
        }
        dval[(int64_t)i * a.ld_dval] = from_f32<T>(d_v);
        dvalT[i] = from_f32<T>(d_v);
    } else if (i < a.Bp) {       // zero the contraction padding of the gradient
        dvalT[i] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vl += __shfl_down(vl, off, 64);
        d_v += __shfl_down(d_v, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = vl;
        red[threadIdx.x >> 6][1] = d_v;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + (threadIdx.x == 0 ? LP_VALUE : LP_DBIAS_V)] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

template <int THREADS = 512>      // (a template: emitted only where it is launched, hgym_update_vf.hip)
__global__ __launch_bounds__(THREADS) void vf_scalars_kernel(const VfScalArgs a) {
    static_assert(THREADS == 16 * LOSS_PARTIALS, "16 partial sums per quantity");
    __shared__ double red[16][LOSS_PARTIALS + 1];
    const int tid = threadIdx.x;
    const int k = tid & (LOSS_PARTIALS - 1), part = tid / LOSS_PARTIALS;      // 512 threads: 16 parts
    const bool vf_k = k == LP_VALUE || k == LP_DBIAS_V;
    const bool bc_k = a.bc_sums && ((k >= LP_DBIAS_MU && k < LP_DBIAS_V) || k == LP_MIRROR);
    const float* __restrict__ partials = a.partials;
    const int nblocks = a.nblocks;
    double s = 0.0;
    if (vf_k) {                  // ppo_scalars_block's order
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int b = part;
        for (; b + 48 < nblocks; b += 64) {
            const float v0 = partials[(int64_t)b * LOSS_PARTIALS + k], v1 = partials[(int64_t)(b + 16) * LOSS_PARTIALS + k];
            const float v2 = partials[(int64_t)(b + 32) * LOSS_PARTIALS + k], v3 = partials[(int64_t)(b + 48) * LOSS_PARTIALS + k];
            s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
        }
        for (; b < nblocks; b += 16) s0 += (double)partials[(int64_t)b * LOSS_PARTIALS + k];
        s = (s0 + s1) + (s2 + s3);
    } else if (bc_k) {           // bc_scalars_kernel's order
        for (int b = part; b < nblocks; b += 16) s += (double)partials[(int64_t)b * LOSS_PARTIALS + k];
    }
    red[part][k] = s;
    __syncthreads();
    if (tid < LOSS_PARTIALS && (vf_k || bc_k)) {
        double t = 0.0;
        for (int p = 0; p < 16; ++p) t += red[p][tid];
        if (tid == LP_VALUE) {
            a.sums[0] += t / a.B;
            a.sums[1] += 1.0;
            if (!a.keep_sqnorm) a.opt[HGYM_OPT_GRAD_SQNORM] = 0.0;      // accumulated by reduce_slabs_kernel later in this call
        } else if (tid == LP_DBIAS_V) {
            if (a.grads_bv) a.grads_bv[0] = (float)t;
        } else if (tid == LP_MIRROR) {
            a.bc_sums[0] += t / ((double)a.B * (double)a.A);
            a.bc_sums[1] += 1.0;
        } else if (a.grads_bmu && tid - LP_DBIAS_MU < a.A) {
            a.grads_bmu[tid - LP_DBIAS_MU] = (float)t;
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers of other translation units
// What hgym_net.hip calls of the files that hold kernels of their own; each of them includes this header, so a drifting signature fails to compile there.
// hgym_update.hip, hgym_update_act.hip: the update's tiles from net `first` on (ELU(1); any resolved activation)
int32_t launch_mlp_fb(const FwdArgs& fb, const FbLoss& fl, bool shadow, bool unclipped, int tiles, int nets, size_t lds, hipStream_t s);
int32_t launch_mlp_fb_act(const FwdArgs& fb, const FbLoss& fl, bool shadow, bool unclipped, int tiles, int nets, hipStream_t s, int first);
// hgym_fwd_act.hip: the fused forward with any resolved activation
int32_t launch_mlp_fwd_act(const FwdArgs& a, int nets, bool wide, int64_t dbg_tiles, hipStream_t s);
// hgym_loss_mirror.hip: ppo_loss_kernel<.., ML = true>
int32_t launch_ppo_loss_mirror(const LossArgs& a, bool bf16, bool unclipped, int nblocks, hipStream_t s);
// hgym_update_bc.hip: the small kernels of hgym_bc_grad
int32_t launch_bc_loss(const BcLossArgs& a, bool bf16, int nblocks, hipStream_t s);
int32_t launch_bc_scalars(const BcScalArgs& a, hipStream_t s);
// hgym_loss_smooth.hip, hgym_smooth.hip: the layer-by-layer head with the smoothness regulariser, the spatial pre-pass's perturbed rows, the sums
int32_t launch_ppo_loss_smooth(const LossArgs& a, const LossSmooth& sm, bool bf16, int nblocks, hipStream_t s);
int32_t launch_perturb_rows(int64_t M, int width, const float* src, int64_t ld_src, const int64_t* idx, const float* noise_std, uint64_t seed,
                            const double* opt_state, float* dst, int64_t ld_dst, hipStream_t s);
int32_t launch_smooth_sums(int nblocks, int B, int A, const float* partials, const float* weight, double* sums, hipStream_t s);
// hgym_loss_mirror_smooth.hip: the layer-by-layer head with both at once, and the sums of the two smoothness terms from head_partials
int32_t launch_ppo_loss_mirror_smooth(const LossArgs& a, const LossSmooth& sm, float* head_partials, bool bf16, int nblocks, hipStream_t s);
int32_t launch_head_sums(int nblocks, int B, int A, const float* head_partials, const float* weight, double* sums, hipStream_t s);
// hgym_guide.hip: the layer-by-layer head with the teacher's term, and the sums of its squared error
int32_t launch_ppo_loss_guide(const LossArgs& a, const LossGuide& gd, bool bf16, int nblocks, hipStream_t s);
int32_t launch_guide_sums(int nblocks, int B, int A, const float* partials, double* sums, hipStream_t s);
// hgym_update_vf.hip: the small kernels of a critic-only step
int32_t launch_vf_loss(const VfLossArgs& a, bool bf16, bool unclipped, int nblocks, hipStream_t s);
int32_t launch_vf_scalars(const VfScalArgs& a, hipStream_t s);

}  // namespace hgym
