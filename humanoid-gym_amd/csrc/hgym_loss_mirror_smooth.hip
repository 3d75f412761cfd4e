// hgym_loss_mirror_smooth.hip -- the small kernels of hgym_ppo_grad_smooth_mirror, in a device code object of their own:
//   ppo_loss_mirror_smooth_kernel<T>   the layer-by-layer path's loss head with the mirror loss AND the smoothness regulariser, fp32 and bf16
//   head_sums_kernel                   the minibatch's two smoothness sums and its weights, from head_partials -> HgymSmooth.sums
// Host code reaches them through launch_ppo_loss_mirror_smooth and launch_head_sums only.
#include "hgym_loss.hpp"

namespace hgym {

// Like ppo_loss_kernel<.., ML = true> and ppo_loss_smooth_kernel it runs BEHIND the plain ppo_loss_kernel on the same arguments and overwrites
// only what the terms change: d mu (row-major and transposed) with all three terms, in the association
//   ((d mu_ppo + g_m (mu - M_a tm)) + gT w (mu - tT)) + gS (mu - tS),
// the LP_DBIAS_MU partials and LP_MIRROR.  The partial row has no slot left for the two smoothness errors: block b writes them to
// hp[4 b], hp[4 b + 1] (HgymSmooth's sums are formed from there).  Each term's expression is the one its own kernel uses.  A kernel of its
// own and not a parameter of either, for the reason given at ppo_loss_smooth_kernel.  A smoothness term whose g is 0 is off and its
// pointers are not read; the mirror loss is always on here.
// fp32 operands: the kernel runs behind ppo_loss_kernel<float, .., ML = true> as well and takes d mu_ppo + g_m (mu - M_a tm) from the d mu
// that kernel left (fp32, exact), adds the two smoothness terms to it and leaves LP_MIRROR alone.  With nothing to round away afterwards
// the first two terms must be the mirror kernel's to the bit (rows that are all done and lamS = 0 give the mirror loss's own gradient),
// and a second compilation of the same expressions does not promise that: measured, it moved 482 of the small test net's 1 397 actor
// gradient words by one unit in the last place.  bf16 operands: all three terms are formed here, behind the plain kernel alone.
template <typename T>
__global__ __launch_bounds__(256) void ppo_loss_mirror_smooth_kernel(const LossArgs a, const LossSmooth sm, float* __restrict__ hp) {
    constexpr bool FROM_ML = sizeof(T) == 4;
    __shared__ float red[4][16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int B = a.b.B, A = a.A;
    const float invB = 1.0f / (float)B;
    float acc[15];               // [0 .. 12) d mu, [12] w |mu - tnext|^2, [13] |mu - tnear|^2, [14] |mu - M_a tm|^2
#pragma unroll
    for (int k = 0; k < 15; ++k) acc[k] = 0.0f;
    T* dmu = (T*)a.dmu;
    T* dmuT = (T*)a.dmuT;
    const bool onT = sm.gT > 0.0f, onS = sm.gS > 0.0f;
    if (i < B) {
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
        if constexpr (!FROM_ML) {
            const int64_t r = a.b.idx[i];
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
        const float wgt = onT ? sm.weight[i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j >= A) continue;
            const float s = sg[j], d = diff[j];
            float g_mu = d_lp * d / (s * s);
            if constexpr (FROM_ML) {
                g_mu = to_f32(dmu[(int64_t)i * a.ld_dmu + j]);      // d mu_ppo + g_m (mu - M_a tm), as the mirror kernel left it
            } else {
                int sj = a.m_src[j];
                sj = sj < 0 ? 0 : (sj >= A ? A - 1 : sj);
                const float dm = rowm[j] - a.m_sign[j] * a.mt[(int64_t)i * A + sj];
                g_mu += a.m_g * dm;
                acc[14] += dm * dm;
            }
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
    for (int k = 0; k < 15; ++k) {
        float s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 15) {
        const float v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        if (k < 12) a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + LP_DBIAS_MU + k] = v;
        else if (k < 14) hp[(int64_t)blockIdx.x * 4 + (k - 12)] = v;
        else if (!FROM_ML) a.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + LP_MIRROR] = v;      // (fp32: the mirror kernel's own)
    }
}

constexpr int HEAD_SUMS_THREADS = 1024;
// smooth_sums_kernel (hgym_smooth.hip) over head_partials' rows of 4 floats instead of the partial row's two slots: the same thread
// count, the same strides over blocks and weights, the same tree -- the same bits for the same partial sums.
__global__ __launch_bounds__(HEAD_SUMS_THREADS) void head_sums_kernel(int nblocks, int B, int A, const float* __restrict__ hp,
                                                                      const float* __restrict__ weight, double* __restrict__ sums) {
    __shared__ double red[3][HEAD_SUMS_THREADS];
    const int tid = threadIdx.x;
    double sT = 0.0, sS = 0.0, sW = 0.0;
    for (int b = tid; b < nblocks; b += HEAD_SUMS_THREADS) {
        sT += (double)hp[(int64_t)b * 4];
        sS += (double)hp[(int64_t)b * 4 + 1];
    }
    if (weight) {
        double w[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int i = tid;
        for (; i + 7 * HEAD_SUMS_THREADS < B; i += 8 * HEAD_SUMS_THREADS) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = weight[i + k * HEAD_SUMS_THREADS];
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] += (double)v[k];
        }
        for (; i < B; i += HEAD_SUMS_THREADS) w[0] += (double)weight[i];
        sW = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
    }
    red[0][tid] = sT;
    red[1][tid] = sS;
    red[2][tid] = sW;
    __syncthreads();
    for (int o = HEAD_SUMS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
            red[2][tid] += red[2][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double inv = 1.0 / ((double)B * (double)A);
        sums[0] += red[0][0] * inv;
        sums[1] += red[1][0] * inv;
        sums[2] += red[2][0];
        sums[3] += 1.0;
    }
}

// (fp32: the caller has launched ppo_loss_kernel<float, .., ML = true> on `a` just before)
int32_t launch_ppo_loss_mirror_smooth(const LossArgs& a, const LossSmooth& sm, float* head_partials, bool bf16, int nblocks, hipStream_t s) {
    if (bf16) hipLaunchKernelGGL((ppo_loss_mirror_smooth_kernel<__bf16>), dim3(nblocks), dim3(256), 0, s, a, sm, head_partials);
    else hipLaunchKernelGGL((ppo_loss_mirror_smooth_kernel<float>), dim3(nblocks), dim3(256), 0, s, a, sm, head_partials);
    HG_CHECK_LAUNCH("ppo_loss_mirror_smooth_kernel");
    return HGYM_OK;
}

// the sums of one minibatch of hgym_ppo_grad_smooth_mirror: rows [0, nblocks) of head_partials, written by the head that has just run
int32_t launch_head_sums(int nblocks, int B, int A, const float* head_partials, const float* weight, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(head_sums_kernel, dim3(1), dim3(HEAD_SUMS_THREADS), 0, s, nblocks, B, A, head_partials, weight, sums);
    HG_CHECK_LAUNCH("head_sums_kernel");
    return HGYM_OK;
}

}  // namespace hgym
