// hgym_smooth.hip -- the streaming kernels of the smoothness regulariser (hgym_ppo_grad_smooth):
//   smooth_pairs_kernel   hgym_smooth_pairs: the successor row and its weight of every row of a permutation
//   perturb_rows_kernel   hgym_perturb_rows: gathered rows plus noise_std * Philox normals, into rows padded to 16 bytes
//   smooth_sums_kernel    the minibatch's two squared-error partials and its weights -> HgymSmooth.sums, in a fixed order
// A translation unit of its own, so that no existing device code object changes.
#include "hgym_fused.hpp"
#include "hgym_loss.hpp"      // (the declaration of what this file defines for hgym_net.hip)

namespace hgym {

constexpr int SMOOTH_THREADS = 256;
constexpr int SMOOTH_MAX_BLOCKS = 4096;      // the kernels loop: a grid never grows with the row count beyond this

__global__ __launch_bounds__(SMOOTH_THREADS) void smooth_pairs_kernel(int64_t B, int64_t N, const int64_t* __restrict__ idx,
                                                                      const uint8_t* __restrict__ dones, int64_t* __restrict__ next_idx,
                                                                      float* __restrict__ next_weight) {
    for (int64_t i = (int64_t)blockIdx.x * SMOOTH_THREADS + threadIdx.x; i < B; i += (int64_t)gridDim.x * SMOOTH_THREADS) {
        const int64_t r = idx[i];
        next_idx[i] = r + N;
        next_weight[i] = dones[r] ? 0.0f : 1.0f;
    }
}

// One lane per (row, four columns): one Philox call (normals_block<1>) covers the lane's columns, the destination leaves as ONE 16-byte
// store (rows of ld_dst floats, ld_dst a multiple of 4, 16-byte aligned base), the source arrives as one 16-byte load at 4-byte alignment
// (F4) -- a source row of 705 floats starts on a 4-byte boundary only; the row's last, partial group is read element by element.
// Columns [width, 4 * ceil(width / 4)) of the destination are written as +0.0; columns from there to ld_dst are not touched.
// A column whose noise_std is 0 is copied, bit for bit (not x + 0 * z: that turns -0.0 into +0.0).
__global__ __launch_bounds__(SMOOTH_THREADS) void perturb_rows_kernel(int64_t M, int width, int G, const float* __restrict__ src, int64_t ld_src,
                                                                      const int64_t* __restrict__ idx, const float* __restrict__ noise_std,
                                                                      uint32_t k0, uint32_t k1, const double* __restrict__ opt,
                                                                      float* __restrict__ dst, int64_t ld_dst) {
    const uint64_t step = (uint64_t)(int64_t)opt[HGYM_OPT_STEP];      // Adam steps taken so far, read before anything of the call advances it
    const RngKey key = {k0, k1, (uint32_t)step, (uint32_t)(step >> 32)};
    const int64_t total = M * (int64_t)G;
    for (int64_t it = (int64_t)blockIdx.x * SMOOTH_THREADS + threadIdx.x; it < total; it += (int64_t)gridDim.x * SMOOTH_THREADS) {
        int64_t m;
        if (total < ((int64_t)1 << 32)) m = (int64_t)((uint32_t)it / (uint32_t)G);
        else m = it / G;
        const int g = (int)(it - m * G);
        const int64_t row = idx ? idx[m] : m;
        const float* __restrict__ x = src + row * ld_src + 4 * g;
        float z[4];
        normals_block<1>(key, (uint32_t)row, SLOT_PERTURB + (uint32_t)g, z);
        float xs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ns[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (4 * g + 3 < width) {      // a whole group: one 16-byte load at 4-byte alignment (F4)
            const F4 qx = *reinterpret_cast<const F4*>(x), qn = *reinterpret_cast<const F4*>(noise_std + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) { xs[e] = qx.v[e]; ns[e] = qn.v[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < width) { xs[e] = x[e]; ns[e] = noise_std[4 * g + e]; }
        }
        float4 o;
        o.x = ns[0] == 0.0f ? xs[0] : __fmaf_rn(ns[0], z[0], xs[0]);
        o.y = ns[1] == 0.0f ? xs[1] : __fmaf_rn(ns[1], z[1], xs[1]);
        o.z = ns[2] == 0.0f ? xs[2] : __fmaf_rn(ns[2], z[2], xs[2]);
        o.w = ns[3] == 0.0f ? xs[3] : __fmaf_rn(ns[3], z[3], xs[3]);
        *reinterpret_cast<float4*>(dst + m * ld_dst + 4 * g) = o;
    }
}

constexpr int SUMS_THREADS = 1024;      // one workgroup of sixteen wavefronts: the weights' loads are latency, not bandwidth
// One workgroup: thread t adds the partial rows t, t + 1024, ... and the weights t, t + 1024, ... in fp64, then the 1024 sums are added in a
// fixed tree -- the same bits whatever the device does in between.
__global__ __launch_bounds__(SUMS_THREADS) void smooth_sums_kernel(int nblocks, int B, int A, const float* __restrict__ partials,
                                                                     const float* __restrict__ weight, double* __restrict__ sums) {
    __shared__ double red[3][SUMS_THREADS];
    const int tid = threadIdx.x;
    double sT = 0.0, sS = 0.0, sW = 0.0;
    for (int b = tid; b < nblocks; b += SUMS_THREADS) {
        sT += (double)partials[(int64_t)b * LOSS_PARTIALS + LP_SMOOTH_T];
        sS += (double)partials[(int64_t)b * LOSS_PARTIALS + LP_SMOOTH_S];
    }
    if (weight) {
        // eight independent loads in flight per thread (a single dependent chain of B / 256 loads on 256 threads took 59 us at B = 61 440, all of it
        // latency); the eight partial sums are combined in a fixed order
        double w[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int i = tid;
        for (; i + 7 * SUMS_THREADS < B; i += 8 * SUMS_THREADS) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = weight[i + k * SUMS_THREADS];
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] += (double)v[k];
        }
        for (; i < B; i += SUMS_THREADS) w[0] += (double)weight[i];
        sW = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
    }
    red[0][tid] = sT;
    red[1][tid] = sS;
    red[2][tid] = sW;
    __syncthreads();
    for (int o = SUMS_THREADS / 2; o > 0; o >>= 1) {
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

static int32_t check_perturb(int64_t M, int32_t width, const float* src, int64_t ld_src, const float* noise_std, const double* opt_state,
                             const float* dst, int64_t ld_dst) {
    HG_REQUIRE(M >= 1 && width >= 1, HGYM_E_BADARG, "hgym_perturb_rows: M=%lld width=%d", (long long)M, width);
    HG_REQUIRE(src && noise_std && opt_state && dst, HGYM_E_BADARG, "hgym_perturb_rows: null src / noise_std / opt_state / dst");
    HG_REQUIRE(ld_src >= width, HGYM_E_BADARG, "hgym_perturb_rows: ld_src=%lld below width=%d", (long long)ld_src, width);
    HG_REQUIRE(ld_dst >= round_up(width, 4) && ld_dst % 4 == 0, HGYM_E_BADARG,
               "hgym_perturb_rows: ld_dst=%lld must be a multiple of 4 and at least %lld", (long long)ld_dst, (long long)round_up(width, 4));
    HG_REQUIRE(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)opt_state & 7) == 0, HGYM_E_BADARG,
               "hgym_perturb_rows: dst must be 16-byte aligned (src 4, opt_state 8)");
    return HGYM_OK;
}

// hgym_perturb_rows behind its checks (hgym_net.hip calls it from hgym_ppo_grad_smooth)
int32_t launch_perturb_rows(int64_t M, int width, const float* src, int64_t ld_src, const int64_t* idx, const float* noise_std, uint64_t seed,
                            const double* opt_state, float* dst, int64_t ld_dst, hipStream_t s) {
    const int32_t rc = check_perturb(M, width, src, ld_src, noise_std, opt_state, dst, ld_dst);
    if (rc) return rc;
    const int G = (width + 3) / 4;
    const int64_t nblk = (M * G + SMOOTH_THREADS - 1) / SMOOTH_THREADS;
    const int blocks = (int)(nblk < SMOOTH_MAX_BLOCKS ? nblk : SMOOTH_MAX_BLOCKS);
    hipLaunchKernelGGL(perturb_rows_kernel, dim3(blocks), dim3(SMOOTH_THREADS), 0, s, M, width, G, src, ld_src, idx, noise_std, (uint32_t)seed,
                       (uint32_t)(seed >> 32), opt_state, dst, ld_dst);
    HG_CHECK_LAUNCH("perturb_rows_kernel");
    return HGYM_OK;
}

// the sums of one minibatch of hgym_ppo_grad_smooth: partial rows [0, nblocks) of the loss head that has just run; weight: null when the
// caller passed none ([2] then gains nothing)
int32_t launch_smooth_sums(int nblocks, int B, int A, const float* partials, const float* weight, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(smooth_sums_kernel, dim3(1), dim3(SUMS_THREADS), 0, s, nblocks, B, A, partials, weight, sums);
    HG_CHECK_LAUNCH("smooth_sums_kernel");
    return HGYM_OK;
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_smooth_pairs(int64_t B, int64_t N, const int64_t* idx, const uint8_t* dones, int64_t* next_idx, float* next_weight, void* stream) {
    HG_REQUIRE(B >= 1 && N >= 1, HGYM_E_BADARG, "hgym_smooth_pairs: B=%lld N=%lld", (long long)B, (long long)N);
    HG_REQUIRE(idx && dones && next_idx && next_weight, HGYM_E_BADARG, "hgym_smooth_pairs: null idx / dones / next_idx / next_weight");
    HG_REQUIRE((((uintptr_t)idx | (uintptr_t)next_idx) & 7) == 0 && ((uintptr_t)next_weight & 3) == 0, HGYM_E_BADARG,
               "hgym_smooth_pairs: idx / next_idx must be 8-byte aligned, next_weight 4-byte");
    const int64_t nblk = (B + SMOOTH_THREADS - 1) / SMOOTH_THREADS;
    const int blocks = (int)(nblk < SMOOTH_MAX_BLOCKS ? nblk : SMOOTH_MAX_BLOCKS);
    hipLaunchKernelGGL(smooth_pairs_kernel, dim3(blocks), dim3(SMOOTH_THREADS), 0, (hipStream_t)stream, B, N, idx, dones, next_idx, next_weight);
    HG_CHECK_LAUNCH("smooth_pairs_kernel");
    return HGYM_OK;
}

int32_t hgym_perturb_rows(int64_t M, int32_t width, const float* src, int64_t ld_src, const int64_t* idx, const float* noise_std, uint64_t seed,
                          const double* opt_state, float* dst, int64_t ld_dst, void* stream) {
    return launch_perturb_rows(M, width, src, ld_src, idx, noise_std, seed, opt_state, dst, ld_dst, (hipStream_t)stream);
}

}  // extern "C"
